"""Device against checker for the power-scaling sensitivity (sbayes_amd.psens, include/sbe_psens.h): the sort against NumPy's
stable argsort on both paths, the sums under the caller's weights against tests/_psens_oracle.py (bound bit for bit where
every gap is a power of two, js within the derived bound, the moments to 1e-14), every output's bits independent of the launch
size, of how rows were appended and of the path, the rules of constant and non-finite columns and vectors, the PSIS weights
against tests/_elpd_oracle.psis_column, and the recorded runs of tests/golden/diag_runs.npz end to end."""
import math
from pathlib import Path

import numpy as np
import pytest

from sbayes_amd import _handle, psens
from tests import _psens_cases as cases
from tests import _psens_oracle as orc

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "diag_runs.npz"
SUMS = ("js", "bound", "js_neg", "bound_neg", "wmean", "wsd")


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _filled(chains, capacity=None):
    chains = [np.ascontiguousarray(c, dtype=np.float64) for c in chains]
    return psens.PsensHandle.filled(None, (len(chains), chains[0].shape[1], capacity or max(len(c) for c in chains)), chains)


def _check_sort(x, path):
    h = _filled([x])
    try:
        h.set_weights(np.ones(len(x)), burnin=0.0)
        assert h.last_shape()[:4] == (1, len(x), 1, path)
        for j in range(x.shape[1]):
            values, samples = h.sorted_column(j)
            xs = x[:, j] + 0.0
            order = np.argsort(xs, kind="stable")
            assert np.array_equal(samples, order), j
            assert _bits(values) == _bits(xs[order]), j
    finally:
        h.close()


@pytest.mark.parametrize("n", cases.SORT_SIZES)
def test_the_sort_is_numpys_stable_argsort(n):
    """Normal draws, three integer values, 0 / 1, zeros of both signs (x + 0.0 folds them), twelve decades, a permutation."""
    _check_sort(cases.columns(n, 300 + n), "lds")


@pytest.mark.parametrize("extra,path", [(0, "lds"), (1, "global")])
def test_the_sort_at_the_edge_between_the_paths(extra, path):
    n = psens.lds_max_draws() + extra
    _check_sort(cases.columns(n, 77)[:, :3], path)


def _compare(got, want, n, label):
    """The flags equal; bound bit for bit where every gap is 0 or 1, within the tree's rounding elsewhere; js within
    orc.bound_js; the moments to 1e-14.  Nothing is left out: a NaN must meet a NaN."""
    assert np.array_equal(got.flag, want["flag"]), (label, got.flag, want["flag"])
    worst = 0.0
    for key, mag in (("js", "magnitude"), ("js_neg", "magnitude_neg")):
        dev, ref = getattr(got, key), want[key]
        assert np.array_equal(np.isnan(dev), np.isnan(ref)), (label, key)
        live = ~np.isnan(ref)
        allowed = orc.bound_js(n, want[mag][live])
        err = np.abs(dev[live] - ref[live])
        if err.size:
            with np.errstate(divide="ignore", invalid="ignore"):
                worst = max(worst, float(np.max(np.where(err == 0.0, 0.0, err / allowed))))
        assert np.all(err <= allowed), (label, key, float(err.max()), float(allowed.min()))
    print(f"[psens-bound] {label}: largest |js - checker| / allowed = {worst:.3g}")
    for key in ("bound", "bound_neg"):
        dev, ref = getattr(got, key), want[key]
        assert np.allclose(dev, ref, rtol=(orc.depth(n) + 2) * 2 * orc.U, atol=0.0, equal_nan=True), (label, key)
    for key in ("wmean", "wsd"):
        assert np.allclose(getattr(got, key), want[key], rtol=1e-14, atol=0.0, equal_nan=True), (label, key)


@pytest.mark.parametrize("v,p,n,launch", [(1, 1, 257, 0), (3, 7, 1000, 2), (16, 7, 300, 0), (3, 7, 5, 2)])
def test_the_sums_under_the_callers_weights(v, p, n, launch):
    x, w = cases.columns(n, 40 + n)[:, :p], cases.weights(v, n, 50 + n)
    h = _filled([x])
    try:
        h.set_launch_columns(launch)
        h.set_weights(w, burnin=0.0)
        got = h.compute()
        chains, draws, vectors, path, launches, per_launch = h.last_shape()
        assert (chains, draws, vectors, path) == (1, n, v, "lds") and launches == (-(-p // launch) if launch else 1)
        assert h.last_kernel_times()[1] > 0.0
    finally:
        h.close()
    want = orc.table(x, w)
    _compare(got, want, n, f"v{v}_p{p}_n{n}")
    for j in (c for c in cases.INTEGER_COLUMNS if c < p):                    # every gap is 0 or 1: no product b P rounds twice
        assert _bits(got.bound[:, j]) == _bits(want["bound"][:, j]) and _bits(got.bound_neg[:, j]) == _bits(want["bound_neg"][:, j]), j
        assert _bits(got.bound[:, j]) == _bits(want["pint"][:, j] + want["qint"][:, j])


def _all_bits(h):
    got = h.compute()
    return {k: _bits(getattr(got, k)) for k in SUMS + ("flag",)}


def test_every_bit_is_independent_of_the_launch_the_appends_and_the_path():
    """Two chains of 180 and 120 rows, 20 and 0 burnt: N = 280 (chunks of 2, the last threads idle)."""
    x = cases.columns(300, 91)
    a, b = x[:180], x[180:]
    w = cases.weights(3, 280, 92)
    burn = [20, 0]
    results = {}
    for label, launch, piece, on_global in (("default", 0, None, False), ("launch_1", 1, None, False), ("launch_2", 2, None, False),
                                            ("rows_1", 0, 1, False), ("rows_3", 0, 3, False), ("global", 0, None, True),
                                            ("global_launch_2", 2, 3, True)):
        h = psens.PsensHandle()
        try:
            h.reset(2, 7, 200)
            for chain, rows in enumerate((a, b)):
                step = piece or len(rows)
                for r0 in range(0, len(rows), step):
                    h.append(chain, rows[r0:r0 + step])
            h.set_launch_columns(launch)
            h.set_global_path(on_global)
            h.set_weights(w, burnin=burn)
            results[label] = _all_bits(h)
            assert h.last_shape()[3] == ("global" if on_global else "lds")
            if label == "default":
                got = h.compute()
        finally:
            h.close()
    for label, bits in results.items():
        assert bits == results["default"], label
    _compare(got, orc.table(orc.stack([a, b], burn), w), 280, "two_chains")


def test_the_edge_sizes_give_the_same_bits_on_both_paths():
    """N = lds_max_draws(): the LDS path by size; the same rows under the switch: the global path."""
    n = psens.lds_max_draws()
    x, w = cases.columns(n, 77)[:, :3], cases.weights(2, n, 78)
    h = _filled([x])
    try:
        h.set_weights(w, burnin=0.0)
        lds = _all_bits(h)
        assert h.last_shape()[3] == "lds"
        h.set_global_path(True)
        assert _all_bits(h) == lds and h.last_shape()[3] == "global"
    finally:
        h.close()


def test_the_rules_of_constant_and_non_finite_columns_and_vectors():
    n = 64
    x = np.array(cases.columns(n, 5)[:, :5])
    x[:, 1] = 2.5                                                            # constant
    x[:, 2] = 1.0 + np.where(np.arange(n) % 2 == 0, 2.0 ** -52, 0.0)       # constant by the rule (max - min < 1e-15), not in its bits
    x[9, 3] = np.nan                                                         # non-finite
    x[:, 4] = -3.0                                                           # a component with equal ratios
    h = _filled([x])
    try:
        with pytest.raises(_handle.EngineError, match="component column 3 holds a non-finite value"):
            h.weights_from_components([0, 3], delta=0.01, burnin=0.0)
        with pytest.raises(_handle.EngineError, match="no weights"):
            h.compute()
        k, ess, vflag, w = h.weights_from_components([0, 4], delta=0.01, burnin=0.0, weights=True)
        got = h.compute()
    finally:
        h.close()
    assert vflag.tolist()[2:] == [psens.VFLAG_CONSTANT] * 2 and not (vflag[:2] & psens.VFLAG_CONSTANT).any()
    assert np.all(w[2:] == 1.0 / n) and np.all(np.isinf(k[2:])) and ess[2:].tolist() == [float(n)] * 2
    assert got.flag.tolist() == [0, psens.FLAG_CONSTANT, psens.FLAG_CONSTANT, psens.FLAG_NONFINITE, psens.FLAG_CONSTANT]
    for key in SUMS:
        assert np.isnan(getattr(got, key)[:, 3]).all(), key
    for key in ("js", "bound", "js_neg", "bound_neg"):
        assert np.all(getattr(got, key)[:, [1, 2, 4]] == 0.0), key
    # the vectors of equal ratios: exact zeros, the bound and the moments of the unweighted draws
    assert np.all(got.js[2:, 0] == 0.0) and np.all(got.js_neg[2:, 0] == 0.0) and np.all(got.bound[2:, 0] > 0.0)
    want = orc.table(x, w, vflag)
    _compare(got, want, n, "rules")
    assert _bits(got.bound[2:, 0]) == _bits(want["pint"][2:, 0] * 2.0)
    assert abs(got.wmean[2, 0] - x[:, 0].mean()) <= 1e-14 and abs(got.wsd[2, 0] - x[:, 0].std()) <= 1e-14
    assert np.all(got.cjs()[2:, [0, 1, 2, 4]] == 0.0) and np.isnan(got.cjs()[:, 3]).all()


def test_unequal_chains_with_their_own_burn_in():
    x = cases.columns(64, 6)
    chains, burn = [x[:40], x[40:52], x[52:]], [7, 0, 8]                     # 33 + 12 + 4 draws
    w = cases.weights(2, 49, 8)
    h = _filled(chains)
    try:
        h.set_weights(w, burnin=burn)
        got = h.compute()
        assert h.last_shape()[:3] == (3, 49, 2)
        stacked = orc.stack(chains, burn)
        values, samples = h.sorted_column(0)
        assert np.array_equal(samples, np.argsort(stacked[:, 0], kind="stable")) and _bits(values) == _bits(np.sort(stacked[:, 0]))
        short = np.array([7, 0, 9], dtype=np.int64)                          # (the library's own refusal: the module refuses earlier)
        with pytest.raises(_handle.EngineError, match="chain 2 has 3 draws after burn-in"):
            h._check(h._lib.sbe_psens_set_weights(h._h, short.ctypes.data, 2, w.ctypes.data))
        with pytest.raises(ValueError, match=r"weights must be \[V, 48\]"):
            h.set_weights(w, burnin=[8, 0, 8])
    finally:
        h.close()
    _compare(got, orc.table(stacked, w), 49, "unequal_chains")


@pytest.mark.parametrize("n,g", [(4, 1), (25, 1), (25, 8), (1000, 1), (1000, 8)])
def test_the_psis_weights_against_the_elpd_checker(n, g):
    """Log weights and k at the tolerance tests/test_gpu_elpd.py uses for the same algorithm: rtol 1e-10, atol 1e-10.  Eight
    components: normal, grid-rounded (equal ratios in the tail) and heavy-tailed columns, by turns."""
    kinds = ("ties", "normal", "heavy")
    x = np.stack([cases.ratios(n, 500 + c, kinds[c % 3]) for c in range(8)], axis=1)
    columns = list(range(g)) if g > 1 else [0]
    delta = 0.01
    h = _filled([x])
    try:
        k, ess, vflag, w = h.weights_from_components(columns, delta=delta, burnin=0.0, weights=True)
        assert h.last_kernel_times()[0] > 0.0 and h.last_shape()[:3] == (1, n, 2 * g)
    finally:
        h.close()
    lws, ks, want_ess, flags = orc.component_weights(x, columns, delta)
    assert np.array_equal(vflag, flags), (vflag, flags)
    assert np.all(w > 0.0)
    assert np.allclose(np.log(w), lws, rtol=1e-10, atol=1e-10)
    assert np.array_equal(np.isinf(k), np.isinf(ks)) and np.allclose(k[np.isfinite(ks)], ks[np.isfinite(ks)], rtol=1e-10, atol=1e-10)
    assert np.array_equal(np.isnan(k), np.isnan(ks))
    assert np.allclose(ess, want_ess, rtol=1e-9, atol=0.0)
    if n == 4:
        assert np.isinf(k).all()                                             # a tail of one: raw weights
    if n == 1000 and g == 8:
        rounded = np.exp(lws[1])                                             # the grid-rounded column at alpha > 1: equal weights among the largest
        assert len(np.unique(np.sort(rounded)[-20:])) < 20


def test_the_psis_weights_give_the_same_bits_on_both_paths():
    kinds = ("ties", "normal", "heavy")
    x = np.stack([cases.ratios(1000, 500 + c, kinds[c % 3]) for c in range(8)], axis=1)
    h = _filled([x])
    try:
        lds = h.weights_from_components(list(range(8)), delta=0.01, burnin=0.0, weights=True)
        assert h.last_shape()[3] == "lds"
        h.set_global_path(True)
        scratch = h.weights_from_components(list(range(8)), delta=0.01, burnin=0.0, weights=True)
        assert h.last_shape()[3] == "global"
    finally:
        h.close()
    for a, b in zip(lds, scratch):
        assert _bits(a) == _bits(b)


WEIGHT_EPS = 2e-10                       # what rtol 1e-10 and atol 1e-10 on a log weight leave of a weight, relatively


def _distance_slack(js, bound, slack):
    """How far sqrt(js / bound) can move when js moves by at most `slack` (js >= 0): the square root is steepest at 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        moved = np.sqrt((js + slack) / bound) - np.sqrt(np.maximum(js - slack, 0.0) / bound)
    return np.where(bound == 0.0, 0.0, moved) + 4 * orc.U


def test_the_recorded_runs_end_to_end():
    """The two recorded runs (60 rows each, all six logged components present): the sensitivities and the diagnosis against the
    checker's, on the first 60 and the last 20 columns.  The device's weights differ from the checker's by what the PSIS
    tolerance allows (WEIGHT_EPS of a weight), which moves every Q_i and M_i by at most 2 WEIGHT_EPS relatively and js by at
    most 8 WEIGHT_EPS A (the derivative of Q log2(Q / M) is bounded by the logs that A sums, plus 1 / ln 2); the square root
    then spreads that over the distance."""
    g = np.load(GOLDEN)
    names = [str(v) for v in g["names"]]
    keep = list(range(60)) + list(range(len(names) - 20, len(names)))
    names = [names[j] for j in keep]
    runs = [g["stats_0"][:, keep], g["stats_1"][:, keep]]
    delta = 0.01
    res = psens.powerscale_sensitivity(runs, names=names, burnin=0.1, delta=delta)
    assert res.components == list(psens.DEFAULT_COMPONENTS) and (res.n_chains, res.n_draws, res.path) == (2, 108, "lds")
    stacked = orc.stack(runs, [6, 6])
    sens, rows, table, ks, flags = orc.powerscale(stacked, res.component_columns, delta)
    assert np.array_equal(res.flag, table["flag"]) and np.array_equal(res.vflag, flags)
    assert np.allclose(res.pareto_k, ks, rtol=1e-10, atol=1e-10)
    slack = orc.bound_js(108, table["magnitude"]) + 8 * WEIGHT_EPS * table["magnitude"]
    slack_neg = orc.bound_js(108, table["magnitude_neg"]) + 8 * WEIGHT_EPS * table["magnitude_neg"]
    row_slack = np.maximum(_distance_slack(table["js"], table["bound"], slack), _distance_slack(table["js_neg"], table["bound_neg"], slack_neg))
    assert np.array_equal(np.isnan(res.cjs), np.isnan(rows))
    live = ~np.isnan(rows)
    assert np.all(np.abs(res.cjs - rows)[live] <= row_slack[live])
    sens_slack = (row_slack[0::2] + row_slack[1::2]) / (2.0 * math.log2(1.0 + delta))
    live = ~np.isnan(sens)
    print(f"[psens-golden] largest |sensitivity - checker| = {np.abs(res.sensitivity - sens)[live].max():.3g}, "
          f"largest allowed = {sens_slack[live].max():.3g}, largest sensitivity = {sens[live].max():.3g}")
    assert np.all(np.abs(res.sensitivity - sens)[live] <= sens_slack[live])
    # the diagnosis: the checker's sensitivities under the paper's rule; no value may sit so close to the threshold that the rule
    # could go either way
    prior, lik = res.components.index("prior"), res.components.index("likelihood")
    threshold = psens.DEFAULT_THRESHOLD
    for row in (prior, lik):
        assert np.all(np.abs(sens[row] - threshold)[live[row]] > sens_slack[row][live[row]])
    want = ["prior-data conflict" if a > threshold and b > threshold else "strong prior / weak likelihood" if a > threshold else "-"
            for a, b in zip(sens[prior], sens[lik])]
    assert res.diagnosis() == want
    assert [r[0] for r in res.table()] == names and len(res.worst(5)) == 5
