"""CPU checks of the model comparison's boundary (include/sbe_compare.h, sbayes_amd/compare.py): the symbols are exported and
bound by the module's own prototype table, the limits agree, and bad arguments are refused before the device is touched."""
import ctypes as ct
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from sbayes_amd import compare, elpd
from tests import _abi_header as abi

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / "include" / "sbe_compare.h").read_text()


def test_every_symbol_of_the_header_is_exported_and_bound():
    abi.check_symbols(compare, HEADER, 12)


def test_limits_agree_with_the_header():
    assert abi.macro(HEADER, "SBE_COMPARE_MAX_MODELS") == str(compare.MAX_MODELS) == "32"
    assert abi.macro(HEADER, "SBE_COMPARE_MAX_POINTS") == "(1 << 24)" and compare.MAX_POINTS == 1 << 24
    assert abi.macro(HEADER, "SBE_COMPARE_MAX_REPLICATES") == "(1 << 16)" and compare.MAX_REPLICATES == 1 << 16
    assert abi.macro(HEADER, "SBE_COMPARE_MAX_IMAGE_BYTES") == "(1ll << 32)" and compare.MAX_IMAGE_BYTES == 1 << 32
    assert abi.macro(HEADER, "SBE_COMPARE_BLOCK") == str(compare.BLOCK) == "256"
    assert abi.macro(HEADER, "SBE_COMPARE_CHUNK") == str(compare.CHUNK) == "4096"
    assert abi.macro(HEADER, "SBE_COMPARE_RUN") == str(compare.RUN) == "1024"
    assert abi.macro(HEADER, "SBE_COMPARE_BOOT_CHUNK") == str(compare.BOOT_CHUNK) == "1024"
    assert abi.macro(HEADER, "SBE_COMPARE_CHECK_EVERY") == str(compare.CHECK_EVERY) == "32"
    # the summation rule: a thread adds CHUNK / BLOCK terms, a bootstrap lane BOOT_CHUNK, a lane of the second kernels at most
    # MAX_POINTS / CHUNK / 64 chunk partials, a thread of the bootstrap's column sums MAX_REPLICATES / BLOCK
    assert compare.CHUNK % compare.BLOCK == 0 and compare.CHUNK // compare.BLOCK <= compare.RUN and compare.BOOT_CHUNK <= compare.RUN
    assert compare.MAX_POINTS // compare.CHUNK // 64 <= compare.RUN and compare.MAX_REPLICATES // compare.BLOCK <= compare.RUN
    # the headline shapes fit, the largest models x points does not: M = 32 goes with N <= 2^23
    assert compare.image_bytes(8, 1_000_000) < compare.image_bytes(32, 1 << 23) == compare.MAX_IMAGE_BYTES < compare.image_bytes(32, (1 << 23) + 1)
    assert compare.image_bytes(1, 1) == 2 * compare.CHUNK * 8
    compare._check_shape(16, 1 << 24)
    for shape in [(0, 10), (33, 10), (1, 0), (1, (1 << 24) + 1), (32, 1 << 24)]:
        with pytest.raises(ValueError):
            compare._check_shape(*shape)


def test_every_array_handed_to_the_library_is_bound_to_a_name():
    abi.check_ptr_arguments(compare)


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to create a handle fails the test."""
    def refuse(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(compare.CompareHandle, "__init__", refuse)


def _v(n, value=-2.0):
    return np.full(n, value)


def _wide(n):
    """A vector of a large size that takes no memory (the checks look at sizes before they copy anything)."""
    return np.broadcast_to(np.float64(-2.0), (n,))


def _loo(v):
    return elpd.LooResult(elpd_loo=float(v.sum()), se=0.0, p_loo=1.5, lppd=0.0, n_samples=10, n_data_points=v.size, warning=False, good_k=0.7,
                          loo_i=v, pareto_k=np.zeros(v.size))


def _waic(v):
    return elpd.WaicResult(elpd_waic=float(v.sum()), se=0.0, p_waic=2.5, lppd=0.0, n_samples=10, n_data_points=v.size, warning=True, waic_i=v)


def _with(n, at, value):
    v = _v(n)
    v[at] = value
    return v


BAD_INPUT = [
    ({}, {}, ValueError, r"0 models; a comparison takes 1 \.\. 32"),
    ({f"m{k}": _v(5) for k in range(33)}, {}, ValueError, r"33 models; a comparison takes 1 \.\. 32"),
    ({"a": _v(0)}, {}, ValueError, r"0 pointwise values per model; a comparison takes 1 \.\. 16777216"),
    ({"a": _wide((1 << 24) + 1)}, {}, ValueError, r"16777217 pointwise values per model"),
    ({f"m{k}": _wide(1 << 24) for k in range(32)}, {}, ValueError, r"takes \d+ bytes on the device, the limit is 4294967296"),
    ({"first": _v(5), "second": _v(5), "third": _v(6)}, {}, ValueError, "models 'first' and 'third' differ in length: 5 and 6 pointwise values"),
    ({"a": _v(5), "b": _with(5, 3, np.nan)}, {}, ValueError, "model 'b': pointwise value 3 is nan, not finite"),
    ({"a": _with(4, 0, -np.inf)}, {}, ValueError, "model 'a': pointwise value 0 is -inf"),
    ({"a": _v(5).astype(np.float32)}, {}, TypeError, "model 'a': the pointwise values must be float64, got float32"),
    ({"a": np.zeros((5, 2))}, {}, ValueError, "must be a vector"),
    ({"a": _loo(_v(5)), "b": _v(5), "c": _waic(_v(5))}, {}, ValueError, r"models 'a' \(LOO\) and 'c' \(WAIC\) mix the two criteria"),
    ({"a": _v(5)}, dict(method="bb-pseudo-bma", alpha=0.5), ValueError, "alpha=0.5"),
    ({"a": _v(5)}, dict(method="bb-pseudo-bma", b_samples=0), ValueError, r"b_samples=0 out of range \[1, 65536\]"),
    ({"a": _v(5)}, dict(method="bb-pseudo-bma", b_samples=(1 << 16) + 1), ValueError, "b_samples=65537 out of range"),
    ({"a": _v(5)}, dict(tol=0.0), ValueError, "tol=0.0 must be positive"),
    ({"a": _v(5)}, dict(tol=-1e-8), ValueError, "must be positive"),
    ({"a": _v(5)}, dict(tol=float("nan")), ValueError, "must be positive"),
    ({"a": _v(5)}, dict(max_iter=0), ValueError, "max_iter=0 out of range"),
    ({"a": _v(5)}, dict(seed=-1), ValueError, "seed=-1"),
    ({"a": _v(5)}, dict(method="bma"), ValueError, "method='bma' is none of stacking, bb-pseudo-bma, pseudo-bma"),
    ([_v(5)], {}, TypeError, "models must be a dict"),
]


@pytest.mark.parametrize("models,kw,err,match", BAD_INPUT)
def test_bad_input_is_refused_before_the_device(no_device, models, kw, err, match):
    with pytest.raises(err, match=match):
        compare.compare(models, **kw)


def test_the_kind_the_p_column_and_the_warnings_are_read_from_the_results():
    names, vectors, kind, p, warning = compare._check_models({"a": _loo(_v(5)), "b": _v(5), "c": _loo(_v(5, -3.0))})
    assert names == ["a", "b", "c"] and kind == "loo" and p[0] == 1.5 and np.isnan(p[1]) and warning == [False, False, False]
    assert all(v.dtype == np.float64 and v.shape == (5,) for v in vectors)
    assert compare._check_models({"w": _waic(_v(3))})[2:] == ("waic", [2.5], [True])
    assert compare._check_models({"v": _v(3)})[2] == "elpd"


def test_c_abi_validates_before_the_device():
    assert sorted(abi.check_null_handles(compare)) == sorted(set(compare.PROTOTYPES) - {"sbe_compare_abi_version", "sbe_compare_last_error"})


def test_handles_are_not_picklable():
    abi.check_not_picklable(compare.CompareHandle)


def test_a_handle_checks_its_own_arguments_before_the_library():
    h = object.__new__(compare.CompareHandle)
    h._h = ct.c_void_p()

    def refuse(*a, **k):
        raise AssertionError("the device was touched")
    h._lib = SimpleNamespace(**{name: refuse for name in compare.PROTOTYPES})
    h.n_models, h.n_points = 3, 10
    for args, match in [((0, 10), "0 models"), ((33, 10), "33 models"), ((2, 0), "0 pointwise values"), ((2, (1 << 24) + 1), "16777217 pointwise"),
                        ((32, 1 << 24), "bytes on the device")]:
        with pytest.raises(ValueError, match=match):
            h.reset(*args)
        h.n_models, h.n_points = 3, 10
    with pytest.raises(ValueError, match=r"model 3 out of range \[0, 3\)"):
        h.set_model(3, _v(10))
    with pytest.raises(ValueError, match="the store holds vectors of 10"):
        h.set_model(0, _v(11))
    with pytest.raises(ValueError, match="model -1 out of range"):
        h.differences(-1)
    for tol in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="must be positive and finite"):
            h.stacking(tol=tol)
    for max_iter in (0, 1 << 31, 2.5, True):
        with pytest.raises(ValueError, match="max_iter="):
            h.stacking(max_iter=max_iter)
    for b in (0, (1 << 16) + 1, 1.5):
        with pytest.raises(ValueError, match="b_samples="):
            h.bootstrap(0, b)
    for alpha in (0.5, 2, 0):
        with pytest.raises(ValueError, match="alpha="):
            h.bootstrap(0, 10, alpha=alpha)
    with pytest.raises(ValueError, match="seed="):
        h.bootstrap(1 << 64, 10)
    h.n_models = 0
    for call in (h.totals, lambda: h.differences(0), h.stacking, h.bootstrap):
        with pytest.raises(ValueError, match="no shape yet"):
            call()


def test_the_result_prints_as_a_table():
    res = compare.CompareResult(names=["K4", "K3"], rank=np.arange(2), elpd=np.array([-10.5, -12.0]), p=np.array([3.25, np.nan]),
                                elpd_diff=np.array([0.0, 1.5]), weight=np.array([0.75, 0.25]), se=np.array([1.0, 2.0]), dse=np.array([0.0, 0.5]),
                                warning=np.array([False, True]), order=np.array([1, 0]), method="stacking", criterion="loo")
    assert res.header() == ["model", "rank", "elpd_loo", "p_loo", "elpd_diff", "weight", "se", "dse", "warning", "scale"]
    row = res.table()[1]
    assert row[:3] + row[4:] == ["K3", 1, -12.0, 1.5, 0.25, 2.0, 0.5, True, "log"] and np.isnan(row[3])
    assert res.table()[0] == ["K4", 0, -10.5, 3.25, 0.0, 0.75, 1.0, 0.0, False, "log"]
    assert res.text() == ("model\trank\telpd_loo\tp_loo\telpd_diff\tweight\tse\tdse\twarning\tscale\n"
                          "K4\t0\t-10.5\t3.25\t0\t0.75\t1\t0\tFalse\tlog\nK3\t1\t-12\tnan\t1.5\t0.25\t2\t0.5\tTrue\tlog\n")


def test_the_command_line_skips_what_it_cannot_use_with_a_warning(tmp_path, monkeypatch, capsys):
    """A file that cannot be read, or whose runs differ in length, is left out with a warning, as sbayes/tools/elpd.py:82-89 does."""
    lengths = {"likelihood_K1_0.npz": 6, "likelihood_K2_0.npz": 6, "likelihood_K3_0.npz": 7}
    for name, n in lengths.items():
        (tmp_path / "exp" / name[11:13]).mkdir(parents=True, exist_ok=True)
        np.savez(tmp_path / "exp" / name[11:13] / name, likelihood=np.full((4, n), 0.5, dtype=np.float32))
    (tmp_path / "exp" / "K4").mkdir()
    (tmp_path / "exp" / "K4" / "likelihood_K4_0.npz").write_bytes(b"not an archive")
    monkeypatch.setattr(elpd, "psis_loo", lambda lh, na_values=None, burnin=0.1, device=None: _loo(np.log(lh[0].astype(np.float64))))
    seen = {}

    def fake(models, **kw):
        seen.update(models)
        return compare.CompareResult(names=list(models), rank=np.arange(2), elpd=np.zeros(2), p=np.zeros(2), elpd_diff=np.zeros(2),
                                     weight=np.full(2, 0.5), se=np.zeros(2), dse=np.zeros(2), warning=np.zeros(2, bool), order=np.arange(2),
                                     method="stacking", criterion="loo")
    monkeypatch.setattr(compare, "compare", fake)
    with pytest.warns(UserWarning) as caught:
        assert compare.main([str(tmp_path)]) == 0
    messages = sorted(str(w.message) for w in caught)
    assert len(messages) == 2 and "likelihood_K4_0.npz'; it is left out" in messages[0] and "likelihood_K3_0.npz' holds 7 observations, the runs before it 6" in messages[1]
    assert list(seen) == ["K1_0", "K2_0"] and capsys.readouterr().out.startswith("exp: 2 runs, stacking")


def test_the_results_folder_is_walked_as_the_reference_tool_walks_it(tmp_path):
    for rel in ["exp1/K2/likelihood_K2_0.npz", "exp1/K2/likelihood_K2_1.npz", "exp1/K3/likelihood_K3_0.h5", "exp1/K3/likelihood_K3_0.chain1.h5",
                "exp2/K1/likelihood_K1_10.npz", "exp2/K1/stats_K1_10.txt", "exp2/other/likelihood_K1_0.npz"]:
        (tmp_path / rel).parent.mkdir(parents=True, exist_ok=True)
        (tmp_path / rel).write_bytes(b"")
    found = compare.find_runs(tmp_path)
    assert {e: [(k, r, p.name) for k, r, p in runs] for e, runs in found.items()} == {
        "exp1": [(2, 0, "likelihood_K2_0.npz"), (2, 1, "likelihood_K2_1.npz"), (3, 0, "likelihood_K3_0.h5")],
        "exp2": [(1, 10, "likelihood_K1_10.npz")]}
