"""On-device screening of all feature pairs (sbayes_amd.assoc, include/sbe_assoc.h) against tests/_assoc_oracle.py and
against what pandas and SciPy returned (tests/golden/assoc.npz): integers equal, the statistic at its derived bound,
the p-value against scipy.special.chdtrc at the device's own statistic and end to end; the table kernel as an
independent check of the matrix-pipe counts; bit-identical results for any launch chunking; limits and errors."""
import ctypes as ct
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from sbayes_amd import assoc
from sbayes_amd.engine import EngineError
from tests import _assoc_oracle as ao

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
CASES = ["south_america", "ragged", "binary", "duplicated", "edge_s32", "edge_one_object", "edge_ragged_n", "edge_two_features"]
FIELDS = ("statistic", "pvalue", "dof", "n", "valid")


@pytest.fixture(scope="module")
def golden():
    with np.load(REPO / "tests" / "golden" / "assoc.npz", allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _case(golden, name):
    return {k[len(name) + 1:]: v for k, v in golden.items() if k.startswith(name + "_")}


def _same_bits(a, b):
    return all(getattr(a, f).tobytes() == getattr(b, f).tobytes() for f in FIELDS)


def _against_oracle(res, r, label):
    """Integers equal; the statistic within (8 + R C) 2^-52; the p-value against the oracle's within the p-value bound
    plus the statistic's share."""
    assert np.array_equal(res.valid, r["valid"]) and np.array_equal(res.dof, r["dof"]) and np.array_equal(res.n, r["n"])
    for f in FIELDS[:1] + FIELDS[2:]:
        assert np.array_equal(getattr(res, f), getattr(res, f).T), f
    v = r["valid"]
    assert np.all(np.isnan(res.pvalue[~v])) and np.all(res.statistic[~v] == 0)
    want = r["statistic"][v]
    err = np.abs(res.statistic[v] - want)
    print(f"{label}: {int(v.sum()) // 2} valid pairs, statistic against the oracle: largest relative difference "
          f"{float(np.max(err / np.maximum(want, ao.DBL_MIN))) if err.size else 0:.3g}")
    assert np.all(err <= ao.statistic_bound(r["R"], r["C"])[v] * want)
    wp = r["pvalue"][v]
    tiny = wp < ao.DBL_MIN
    assert np.all((res.pvalue[v][tiny] >= 0) & (res.pvalue[v][tiny] < ao.DBL_MIN))
    pb = ao.pvalue_bound_end_to_end(r["statistic"], r["R"], r["C"])[v]
    perr = np.abs(res.pvalue[v] - wp)
    print(f"{label}: p-value against the oracle: largest relative difference "
          f"{float(np.max((perr / np.maximum(wp, ao.DBL_MIN))[~tiny])) if (~tiny).any() else 0:.3g}")
    assert np.all(perr[~tiny] <= (2 * pb * wp)[~tiny])            # (both sides carry the p-value bound)


@pytest.mark.parametrize("name", CASES)
def test_device_against_oracle_and_fixture(golden, name):
    special = pytest.importorskip("scipy.special")
    c = _case(golden, name)
    res = assoc.feature_association(c["x"], c["n_states"])
    r = ao.feature_association(c["x"], c["n_states"])
    _against_oracle(res, r, name)
    # the fixture: what pd.crosstab + chi2_contingency returned
    keep = ~c["skipped"]
    assert np.array_equal(ao.upper(res.valid), keep)
    assert np.array_equal(ao.upper(res.dof), c["dof"]) and np.array_equal(ao.upper(res.n), c["n"])
    stat, want = ao.upper(res.statistic)[keep], c["statistic"][keep]
    sb = ao.statistic_bound(ao.upper(r["R"]), ao.upper(r["C"]))[keep]
    if stat.size:
        print(f"{name}: statistic against SciPy: largest relative difference {float(np.max(np.abs(stat - want) / np.maximum(want, ao.DBL_MIN))):.3g}")
    assert np.all(np.abs(stat - want) <= sb * want)
    # the p-value, step 1: against chdtrc evaluated at the device's own statistic
    pv = ao.upper(res.pvalue)[keep]
    own = special.chdtrc(ao.upper(res.dof)[keep], stat)
    normal = own >= ao.DBL_MIN
    assert np.all((pv[~normal] >= 0) & (pv[~normal] < ao.DBL_MIN))
    if normal.any():
        print(f"{name}: p-value against chdtrc at the device's statistic: largest relative error "
              f"{float(np.max(np.abs(pv - own)[normal] / own[normal])):.3g} (bound {ao.PVALUE_BOUND:.3g})")
    assert np.all(np.abs(pv - own)[normal] <= ao.PVALUE_BOUND * own[normal])
    # step 2: end to end against the fixture
    wp = c["pvalue"][keep]
    normal = wp >= ao.DBL_MIN
    assert np.all((pv[~normal] >= 0) & (pv[~normal] < ao.DBL_MIN))
    assert bool((~normal).any()) == (name == "duplicated")
    pb = ao.pvalue_bound_end_to_end(c["statistic"], ao.upper(r["R"]), ao.upper(r["C"]))[keep]
    assert np.all(np.abs(pv - wp)[normal] <= (pb * wp)[normal])


@pytest.mark.parametrize("name", ["south_america", "ragged", "edge_s32", "edge_one_object", "edge_ragged_n", "edge_two_features"])
def test_table_kernel_checks_the_matrix_pipe_counts(golden, name):
    c = _case(golden, name)
    res = assoc.feature_association(c["x"], c["n_states"])
    r = ao.feature_association(c["x"], c["n_states"])
    f = c["x"].shape[1]
    pairs = np.argwhere(np.triu(np.ones((f, f), dtype=bool), 1))
    tabs = res.tables(pairs)
    assert tabs.dtype == np.int32 and tabs.shape == (len(pairs), c["n_states"].max(), c["n_states"].max())
    assert np.array_equal(tabs, r["tables"][pairs[:, 0], pairs[:, 1]])
    for (i, j), t in zip(pairs, tabs):                     # the statistic from the integer tables, on the host
        valid, dof, n, stat, R, C = ao.table_statistic(t)
        assert (valid, dof, n) == (res.valid[i, j], res.dof[i, j], res.n[i, j])
        assert abs(stat - res.statistic[i, j]) <= ao.statistic_bound(R, C) * stat
    swapped = res.tables(pairs[:4, ::-1])                  # (j, i): the transposed table
    assert np.array_equal(swapped, tabs[:4].transpose(0, 2, 1))


def test_results_do_not_depend_on_the_call_or_the_chunking(golden):
    c = _case(golden, "ragged")
    h = assoc.handle_for(0)
    try:
        a = assoc.feature_association(c["x"], c["n_states"])
        s_pad, tile_pairs, launches = h.last_shape()
        assert s_pad == 16 and tile_pairs == 20 * 21 // 2 and launches == 1
        b = assoc.feature_association(c["x"], c["n_states"])
        assert _same_bits(a, b)
        for per_launch in (1, 7, 64):
            h.set_launch_tiles(per_launch)
            d = assoc.feature_association(c["x"], c["n_states"])
            assert h.last_shape() == (16, tile_pairs, -(-tile_pairs // per_launch))
            assert _same_bits(a, d), per_launch
        assert h.last_kernel_ms() > 0
    finally:
        h.set_launch_tiles(0)


@pytest.mark.parametrize("name,s_pad", [("headline", 16), ("stress", 32)])
def test_engine_feature_blocks_against_the_oracle(name, s_pad):
    """The synthetic headline (1000 x 200 x 10) and stress (5000 x 500 x 20) feature blocks, through the one-hot interface."""
    from sbayes_amd.synthetic import make_workload
    features = make_workload(name).features
    res = assoc.feature_association(features)
    assert assoc.handle_for(0).last_shape()[0] == s_pad
    x = assoc.state_codes(features)
    assert np.array_equal(res.n_states, np.full(x.shape[1], features.shape[2]))
    _against_oracle(res, ao.feature_association(x, res.n_states), name)


def test_result_object_on_south_america(golden):
    c = _case(golden, "south_america")
    onehot = np.zeros(c["x"].shape + (int(c["n_states"].max()),), dtype=bool)
    i, j = np.nonzero(c["x"] != ao.NA)
    onehot[i, j, c["x"][i, j]] = True
    res = assoc.feature_association(onehot)
    codes = assoc.feature_association(c["x"], c["n_states"])
    assert _same_bits(res, codes)                          # states that never occur change nothing
    flagged = res.correlated()
    assert len(flagged) == 40 and flagged == sorted(flagged) and abs(flagged[0][0] - 9.2e-12) < 1e-13
    iu = np.triu_indices(36, 1)
    want = sorted((p, a, b) for p, a, b in zip(c["pvalue"], *iu) if p < 1e-4)
    assert [(a, b) for _p, a, b in flagged] == [(a, b) for _p, a, b in want]
    _p, a, b = flagged[0]
    observed, expected, deviation = res.table(a, b)
    assert observed.sum() == res.n[a, b] and observed.shape == expected.shape and min(observed.shape) > 1
    assert (observed.shape[0] - 1) * (observed.shape[1] - 1) == res.dof[a, b]
    assert np.allclose(expected.sum(axis=0), observed.sum(axis=0)) and np.allclose(deviation.sum(), 0, atol=1e-9)


def test_command_line_prints_the_tools_report(golden, tmp_path, capsys):
    pytest.importorskip("pandas")
    c = _case(golden, "south_america")
    letters = "ABCDEFGH"
    lines = ["name,id,x,y,family," + ",".join(f"F{k + 1}" for k in range(36))]
    for n, row in enumerate(c["x"]):
        lines.append(f"L{n},l{n},0.0,0.0,," + ",".join("" if v == ao.NA else letters[v] for v in row))
    path = tmp_path / "features.csv"
    path.write_text("\n".join(lines) + "\n")
    assert assoc.main(["--input", str(path)]) == 0
    out = capsys.readouterr().out.splitlines()
    assert out[0] == "(100, 36)"
    assert sum(ln.startswith("Correlation between [") for ln in out) == 40
    assert sum(ln.startswith("Chi-squared test p-value = ") for ln in out) == 40
    assert assoc.main(["--input", str(path), "-p", "1e-30"]) == 0
    assert capsys.readouterr().out.splitlines() == ["(100, 36)"]


def test_limits_and_errors_at_the_c_boundary():
    lib = assoc.load()
    h = ct.c_void_p()
    assert lib.sbe_assoc_create(ct.byref(h), 0) == 0 and h
    try:
        x = np.zeros((8, 3), dtype=np.uint8)
        ns = np.array([2, 2, 2], dtype=np.int32)
        f8, i4, u1 = np.zeros((2, 9)), np.zeros((2, 9), dtype=np.int32), np.zeros(9, dtype=np.uint8)
        outs = [a.ctypes.data for a in (f8[0], f8[1], i4[0], i4[1], u1)]
        err = lambda: lib.sbe_assoc_last_error(h).decode()       # noqa: E731
        pairs = np.array([[0, 1]], dtype=np.int32)
        tab = np.zeros((1, 2, 2), dtype=np.int32)
        assert lib.sbe_assoc_tables(h, pairs.ctypes.data, 1, tab.ctypes.data) == 3 and "sbe_assoc_compute" in err()     # SBE_ERR_STATE
        ns33 = np.array([2, 33, 2], dtype=np.int32)
        assert lib.sbe_assoc_compute(h, x.ctypes.data, 8, 3, ns33.ctypes.data, *outs) == 1
        assert "n_states[1]=33" in err() and "[1, 32]" in err()
        assert lib.sbe_assoc_compute(h, x.ctypes.data, (1 << 24) + 1, 3, ns.ctypes.data, *outs) == 1      # (argument check only)
        assert "n_objects=16777217" in err() and "2^24" in err()
        assert lib.sbe_assoc_compute(h, x.ctypes.data, 8, 4097, ns.ctypes.data, *outs) == 1
        assert "n_features=4097" in err() and "4096" in err()
        assert lib.sbe_assoc_compute(h, x.ctypes.data, 1 << 20, 4096, ns.ctypes.data, *outs) == 1
        assert "2^31" in err()
        bad = x.copy()
        bad[5, 2] = 2
        assert lib.sbe_assoc_compute(h, bad.ctypes.data, 8, 3, ns.ctypes.data, *outs) == 4                # SBE_ERR_DATA
        assert "x[5][2]=2" in err() and "n_states[2]=2" in err()
        assert lib.sbe_assoc_compute(h, None, 8, 3, ns.ctypes.data, *outs) == 1 and "null pointer argument: x" in err()
        assert lib.sbe_assoc_compute(h, x.ctypes.data, 8, 3, None, *outs) == 1 and "n_states" in err()
        assert lib.sbe_assoc_compute(h, x.ctypes.data, 8, 3, ns.ctypes.data, outs[0], None, *outs[2:]) == 1 and "output" in err()
        assert lib.sbe_assoc_set_launch_tiles(h, -1) == 1
        s_pad, tiles, launches = ct.c_int32(), ct.c_int64(), ct.c_int64()
        assert lib.sbe_assoc_last_shape(h, ct.byref(s_pad), ct.byref(tiles), ct.byref(launches)) == 3     # nothing was launched
        assert lib.sbe_assoc_compute(h, x.ctypes.data, 8, 3, ns.ctypes.data, *outs) == 0
        assert not u1.any() and np.all(np.isnan(f8[1]))               # one state everywhere: no pair can be tested
        assert lib.sbe_assoc_tables(h, pairs.ctypes.data, 1, tab.ctypes.data) == 0 and tab[0, 0, 0] == 8 and tab.sum() == 8
        pairs[0, 1] = 3
        assert lib.sbe_assoc_tables(h, pairs.ctypes.data, 1, tab.ctypes.data) == 1 and "pairs[0][1]=3" in err()
        assert lib.sbe_assoc_tables(h, None, 1, tab.ctypes.data) == 1 and "null pointer" in err()
    finally:
        assert lib.sbe_assoc_destroy(h) == 0


def test_python_layer_names_the_device_limit():
    with pytest.raises(EngineError, match="2\\^31"):
        h = assoc.handle_for(0)
        x = np.broadcast_to(np.zeros((1, 1), dtype=np.uint8), (1 << 20, 4096))
        h.compute(x, np.ones(4096, dtype=np.int32))


_FORK_PROBE = r"""
import json, os, sys
sys.path.insert(0, {repo!r})
import numpy as np
from sbayes_amd import _proc, assoc

x = (np.arange(200).reshape(50, 4) % 3).astype(np.uint8)
before = assoc.feature_association(x)
h = assoc.handle_for(0)
handle = h._h.value
r, w = os.pipe()
pid = os.fork()
if pid == 0:                                  # child: NO HIP call is made here
    os.close(r)
    out = dict(cache_empty=not assoc._HANDLES, handle_nulled=not bool(h._h))
    for tag, fn in (("inherited", lambda: h.compute(x, before.n_states)),
                    ("create", lambda: assoc.feature_association(x)),
                    ("tables", lambda: before.tables([(0, 1)]))):
        try:
            fn()
            out[tag] = "no error"
        except (_proc.ForkedWithHipError, RuntimeError) as exc:
            out[tag] = type(exc).__name__ + ": " + str(exc)
    os.write(w, json.dumps(out).encode())
    os._exit(0)
os.close(w)
child = json.loads(os.read(r, 1 << 16).decode())
_, status = os.waitpid(pid, 0)
after = assoc.feature_association(x)
print(json.dumps(dict(child=child, status=status, same=before.statistic.tobytes() == after.statistic.tobytes(),
                      same_handle=h._h.value == handle)))
assoc.release_all()
"""


def test_forked_child_forgets_the_handle():
    res = subprocess.run([sys.executable, "-c", _FORK_PROBE.format(repo=str(REPO))], capture_output=True, text=True,
                         timeout=600, cwd=str(REPO))
    assert res.returncode == 0, res.stderr[-3000:]
    out = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
    child = out["child"]
    assert out["status"] == 0 and out["same"] and out["same_handle"]
    assert child["cache_empty"] and child["handle_nulled"]
    assert child["inherited"].startswith("ForkedWithHipError") and "fork()" in child["inherited"]
    assert child["create"].startswith("ForkedWithHipError") and "forkserver" in child["create"]
    assert "error" in child["tables"].lower() and child["tables"] != "no error"
