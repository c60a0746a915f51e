"""CPU checks of the sensitivity boundary (include/sbe_psens.h, sbayes_amd/psens.py): the symbols are exported and bound by the
module's own prototype table, the limits agree, and bad arguments are refused before the device is touched."""
import ctypes as ct
import dataclasses
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from sbayes_amd import diag, psens
from tests import _abi_header as abi
from tests import _psens_oracle as orc

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / "include" / "sbe_psens.h").read_text()


def test_every_symbol_of_the_header_is_exported_and_bound():
    names = abi.check_symbols(psens, HEADER, 17)
    assert not set(names) & set(diag.PROTOTYPES)


def test_limits_and_codes_agree_with_the_header():
    assert abi.macro(HEADER, "SBE_PSENS_MAX_COMPONENTS") == str(psens.MAX_COMPONENTS) == "8"
    assert abi.macro(HEADER, "SBE_PSENS_MAX_VECTORS") == str(psens.MAX_VECTORS) == "16" and psens.MAX_VECTORS == 2 * psens.MAX_COMPONENTS
    assert (int(abi.macro(HEADER, "SBE_PSENS_VFLAG_CONSTANT")), int(abi.macro(HEADER, "SBE_PSENS_VFLAG_UNRELIABLE"))) == \
        (psens.VFLAG_CONSTANT, psens.VFLAG_UNRELIABLE) == (orc.VFLAG_CONSTANT, orc.VFLAG_UNRELIABLE)
    # the limits of the diagnostics are the sensitivity's own
    assert (psens.MAX_CHAINS, psens.MIN_DRAWS, psens.MAX_DRAWS, psens.MAX_COLUMNS) == (diag.MAX_CHAINS, diag.MIN_DRAWS, diag.MAX_DRAWS, diag.MAX_COLUMNS)
    assert (psens.FLAG_CONSTANT, psens.FLAG_NONFINITE) == (orc.FLAG_CONSTANT, orc.FLAG_NONFINITE)
    # the sort keys of the longest column kept in LDS (12 bytes a draw) and the kernels' static LDS fit the 160 KiB of a CU, and
    # one more draw would not
    assert psens.lds_max_draws() * 12 + 8192 <= 160 * 1024 < (psens.lds_max_draws() + 1) * 12 + 8192
    assert len(psens.DEFAULT_COMPONENTS) <= psens.MAX_COMPONENTS and psens.DEFAULT_DELTA > 0.0


def test_every_array_handed_to_the_library_is_bound_to_a_name():
    abi.check_ptr_arguments(psens)


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to create a handle fails the test."""
    def refuse(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(psens.PsensHandle, "__init__", refuse)


NAMES = ["likelihood", "prior", "x"]


@pytest.mark.parametrize("chains,kw,err,match", [
    ([], {}, ValueError, r"0 chains; the diagnostics take 1 \.\. 64"),
    (np.zeros((65, 10, 3)), {}, ValueError, "65 chains"),
    (np.zeros((10, 3)), {}, ValueError, r"\[M, S, P\]"),
    ([np.zeros((10, 3)), np.zeros((10, 2))], {}, ValueError, "unequal column counts"),
    ([np.zeros((10, 3))], dict(components=[]), ValueError, r"0 components; a call takes 1 \.\. 8"),
    ([np.zeros((10, 3))], dict(components=[0] * 9), ValueError, r"9 components; a call takes 1 \.\. 8"),
    ([np.zeros((10, 3))], dict(components=[3]), ValueError, r"component column 3 out of range \[0, 3\)"),
    ([np.zeros((10, 3))], dict(components=[-1]), ValueError, "component column -1 out of range"),
    ([np.zeros((10, 3))], dict(components=["geo_prior"], names=NAMES), ValueError, "component 'geo_prior' is not among the column names"),
    ([np.zeros((10, 3))], dict(components=["prior"]), ValueError, "not among the column names"),
    ([np.zeros((10, 3))], {}, ValueError, "none of the default components"),
    ([np.zeros((10, 3))], dict(names=["a", "b", "c"]), ValueError, "none of the default components"),
    ([np.zeros((10, 3))], dict(components=[0], delta=0.0), ValueError, r"delta=0\.0 must be positive"),
    ([np.zeros((10, 3))], dict(components=[0], delta=-0.01), ValueError, "must be positive"),
    ([np.zeros((10, 3))], dict(components=[0], delta=float("nan")), ValueError, "must be positive"),
    ([np.zeros((10, 3)), np.zeros((3, 3))], dict(components=[0], burnin=0.0), ValueError, "chain 1 has 3 draws after burn-in; at least 4"),
    ([np.zeros((7, 3))], dict(components=[0], burnin=0.6), ValueError, "chain 0 has 3 draws after burn-in; at least 4"),
    ([np.zeros((10, 3))], dict(components=[0], burnin=1.0), ValueError, r"must lie in \[0, 1\)"),
    ([np.zeros((10, 3))], dict(components=[0], burnin=[1, 2]), ValueError, "2 burn-in row counts for 1 chains"),
    ([np.broadcast_to(np.zeros((1, 1)), ((1 << 19) + 1, 1))] * 2, dict(components=[0], burnin=0.0), ValueError, r"exceed 1048576 \(2\^20\)"),
    ([np.zeros((10, 3))], dict(components=[0], names=["a"]), ValueError, "1 names for 3 columns"),
    ([np.zeros((10, 3), dtype="U1")], dict(components=[0], burnin=0.0), TypeError, "numeric"),
])
def test_bad_input_is_refused_before_the_device(no_device, chains, kw, err, match):
    with pytest.raises(err, match=match):
        psens.powerscale_sensitivity(chains, **kw)


def test_default_components_are_those_the_names_hold():
    names = ["Sample", "likelihood", "prior", "geo_prior", "w_a"]
    assert psens._check_components(None, names, 5) == (["likelihood", "prior", "geo_prior"], [1, 2, 3])
    assert psens._check_components(["prior", 4], names, 5) == (["prior", "w_a"], [2, 4])
    assert psens._check_components([1], None, 5) == (["c1"], [1])


def test_c_abi_validates_before_the_device():
    assert sorted(abi.check_null_handles(psens)) == sorted(set(psens.PROTOTYPES) - {"sbe_psens_abi_version", "sbe_psens_last_error",
                                                                                    "sbe_psens_lds_max_draws"})


def test_handles_are_not_picklable():
    abi.check_not_picklable(psens.PsensHandle)


def test_a_handle_checks_its_own_arguments_before_the_library():
    h = object.__new__(psens.PsensHandle)
    h._h = ct.c_void_p()
    h.n_chains, h.n_columns, h.capacity = 2, 3, 10

    def refuse(*a, **k):
        raise AssertionError("the device was touched")
    h._lib = SimpleNamespace(**{name: refuse for name in psens.PROTOTYPES})
    h.rows = lambda chain: 10
    with pytest.raises(ValueError, match=r"65 chains"):
        h.reset(65, 3, 10)
    h.n_chains, h.n_columns = 2, 3
    with pytest.raises(ValueError, match="chain 2 out of range"):
        h.append(2, np.zeros((1, 3)))
    with pytest.raises(ValueError, match="rows have 4 columns, the store has 3"):
        h.append(0, np.zeros((1, 4)))
    with pytest.raises(ValueError, match="0 components"):
        h.weights_from_components([])
    with pytest.raises(ValueError, match="9 components"):
        h.weights_from_components([0] * 9)
    with pytest.raises(ValueError, match="component column 3 out of range"):
        h.weights_from_components([3])
    with pytest.raises(ValueError, match="delta"):
        h.weights_from_components([0], delta=0.0)
    with pytest.raises(ValueError, match="chain 0 has 2 draws after burn-in"):
        h.weights_from_components([0], burnin=[8, 0])
    # 2 chains of 10 rows, a tenth burnt: N = 18
    with pytest.raises(ValueError, match=r"weights must be \[V, 18\]"):
        h.set_weights(np.ones((2, 20)))
    with pytest.raises(ValueError, match=r"weights must be \[V, 18\]"):
        h.set_weights(np.ones((17, 18)))
    with pytest.raises(ValueError, match="non-negative and finite"):
        h.set_weights(-np.ones((1, 18)))
    with pytest.raises(ValueError, match="non-negative and finite"):
        h.set_weights(np.full((1, 18), np.inf))
    with pytest.raises(ValueError, match="positive sum"):
        h.set_weights(np.stack([np.ones(18), np.zeros(18)]))
    with pytest.raises(TypeError, match="numeric"):
        h.set_weights(np.zeros((1, 18), dtype="U1"))
    with pytest.raises(ValueError, match="column 3 out of range"):
        h.sorted_column(3)
    with pytest.raises(ValueError, match="0 values"):
        h.device_log2([])


def test_the_host_part_of_the_contract_is_the_checkers():
    rng = np.random.default_rng(5)
    js, bound, js_neg, bound_neg = (rng.random((4, 6)) for _ in range(4))
    bound[0, 0] = 0.0
    got = psens.cjs_distance(js, bound, js_neg, bound_neg)
    want = orc.cjs(dict(js=js, bound=bound, js_neg=js_neg, bound_neg=bound_neg))
    assert got.tobytes() == want.tobytes() and psens.sensitivity_of(got, 0.01).tobytes() == orc.sensitivity(want, 0.01).tobytes()
    assert psens.distance([0.0], [0.0]).tolist() == [0.0]


def _result(sens, components):
    g, p = sens.shape
    return psens.PsensResult(sensitivity=sens, cjs=np.zeros((2 * g, p)), wmean=np.zeros((2 * g, p)), wsd=np.zeros((2 * g, p)),
                             pareto_k=np.zeros(2 * g), ess=np.ones(2 * g), vflag=np.zeros(2 * g, dtype=np.uint8),
                             flag=np.array([0, 0, 1, 2][:p], dtype=np.uint8), components=components, component_columns=list(range(g)), delta=0.01,
                             names=list("abcd")[:p], n_chains=2, n_draws=10)


def test_diagnosis_table_and_worst():
    sens = np.array([[0.2, 0.01, 0.0, np.nan], [0.3, 0.06, 0.0, np.nan], [0.01, 0.5, 0.0, np.nan]])
    res = _result(sens, ["likelihood", "prior", "geo_prior"])
    assert res.diagnosis() == ["prior-data conflict", "strong prior / weak likelihood", "-", "-"]
    assert res.diagnosis(threshold=0.25) == ["strong prior / weak likelihood", "-", "-", "-"] and res.diagnosis(0.35) == ["-"] * 4
    assert res.diagnosis(0.1)[0] == "prior-data conflict"
    assert res.header() == ["column", "likelihood", "prior", "geo_prior", "diagnosis", "flag"]
    rows = res.table()
    assert rows[1] == ["b", 0.01, 0.06, 0.5, "strong prior / weak likelihood", 0] and all(len(r) == len(res.header()) for r in rows)
    assert res.worst(2) == [("b", "geo_prior", 0.5), ("a", "prior", 0.3)] and len(res.worst(10)) == 4 and res.worst(10)[-1][0] == "d"
    assert _result(sens[:2], ["likelihood", "geo_prior"]).diagnosis() == ["-"] * 4


def test_the_command_line_aligns_the_labels_before_it_stacks_the_columns(tmp_path, monkeypatch, capsys):
    """The files are read through the diagnostics' readers; the two device calls (alignment, sensitivity) are replaced: run 1
    has its labels swapped, and what reaches powerscale_sensitivity must be in run 0's labels, stats and indicators alike."""
    from sbayes_amd import align
    rng = np.random.default_rng(3)
    s, k, n = 12, 2, 5
    clusters0 = np.zeros((s, k, n), dtype=np.uint8)
    clusters0[:, 0, :2], clusters0[:, 1, 3:] = 1, 1
    clusters1 = clusters0[:, ::-1].copy()
    header = ["Sample", "likelihood", "prior", "size_a0", "size_a1", "w_x"]
    rows0 = np.column_stack([np.arange(s), rng.normal(-100, 3, s), rng.normal(-50, 2, s), np.full(s, 2.0), np.full(s, 3.0), rng.random(s)])
    rows1 = rows0.copy()
    rows1[:, [3, 4]] = rows0[:, [4, 3]]
    stats, files = [], []
    for r, (rows, clusters) in enumerate(((rows0, clusters0), (rows1, clusters1))):
        stats.append(str(tmp_path / f"stats_K2_{r}.txt"))
        files.append(str(tmp_path / f"clusters_K2_{r}.txt"))
        align.write_stats_text(stats[-1], header, [[repr(float(v)) for v in row] for row in rows])
        align.write_clusters(files[-1], clusters)
    seen = {}

    def fake_align(samples, device=None):
        assert [c.shape for c in samples] == [(s, k, n)] * 2
        return SimpleNamespace(total_perms=[np.tile([0, 1], (s, 1)), np.tile([1, 0], (s, 1))])

    def fake_sensitivity(runs, components=None, delta=0.01, burnin=0.1, names=None, device=None):
        seen.update(runs=runs, names=names, components=components, delta=delta, burnin=burnin)
        sens = np.array([[0.2] * len(names), [0.3] * len(names)])
        return dataclasses.replace(_result(sens[:, :4], ["likelihood", "prior"]), sensitivity=sens, names=list(names),
                                   flag=np.zeros(len(names), dtype=np.uint8))
    monkeypatch.setattr(align, "align_runs", fake_align)
    monkeypatch.setattr(psens, "powerscale_sensitivity", fake_sensitivity)
    out = tmp_path / "sensitivity.tsv"
    assert psens.main(stats + ["--clusters"] + files + ["--delta", "0.02", "-o", str(out), "--top", "3"]) == 0
    assert seen["names"] == header[1:] + [f"a{c}_{i}" for c in range(k) for i in range(n)] and (seen["delta"], seen["components"]) == (0.02, None)
    assert np.array_equal(seen["runs"][0], seen["runs"][1])                  # run 1 arrived in run 0's labels
    assert np.array_equal(seen["runs"][0][:, 5:], clusters0.reshape(s, -1)) and np.array_equal(seen["runs"][0][:, :5], rows0[:, 1:])
    lines = out.read_text().splitlines()
    assert lines[0].split("\t") == ["column", "likelihood", "prior", "diagnosis", "flag"] and len(lines) == 1 + len(seen["names"])
    assert lines[1].split("\t") == ["likelihood", "0.2", "0.3", "prior-data conflict", "0"]
    assert "prior-data conflict: 15 columns" in capsys.readouterr().out
