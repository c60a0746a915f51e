"""The range cases of the column kernel (tests/_diag_range_cases.py) under the checker alone: that each case reaches the
mechanism it is there for -- rho_t entries past 2048 and which cases write them, a monotone replacement on the boundary,
walks, max_lag stops and stops by the rule on either side of a multiple of 32, the flags at the constant threshold -- and that
every column decides with a margin no rounding of the device can cross.  tests/test_gpu_diag_range.py runs them on the
device."""
import math

import numpy as np
import pytest

from tests import _diag_oracle as orc
from tests import _diag_range_cases as cases
from tests import _summary_oracle as sorc


@pytest.mark.parametrize("name", list(cases.CASES))
def test_every_column_decides_with_a_margin_above_twice_its_rho_bound(name):
    """>= 1e-9 and above twice the bound on a device's rho.  (The fixed cases of tests/_diag_cases.py also keep twice the rho
    bound below 1e-9; a column at 1e9 +- 1 cannot: its rho bound is of the order of 1e-6, against a margin of 1e-3.)"""
    _x, _kw, want = cases.case(name)
    varying = (want["flag"] & orc.FLAG_CONSTANT) == 0
    print(f"[diag-range] {name}: n_lags {want['n_lags'].tolist()} least margin {want['margin'].min():.3g} largest 2 rho bound "
          f"{2 * want['rho_bound'].max():.3g}")
    assert not (want["flag"] & orc.FLAG_NONFINITE).any()
    assert np.all(want["margin"][varying] >= cases.MIN_MARGIN)
    assert np.all(want["margin"][varying] > 2 * want["rho_bound"][varying])
    assert cases.safe(want).all()
    for k in orc.FIELDS:
        b = want["bound"][k]
        assert np.all(b >= 0) and np.all(np.isfinite(b)), k


# ---- A ------------------------------------------------------------------------------------------------------------------
def test_the_allocation_edge_stops_where_it_should():
    """n = 2048: no scratch.  2050: a scratch, but the last entry written is 2047.  2051 and 2052: the smallest n that write
    entries 2048 and 2049."""
    assert cases.ALLOC_N == (2048, 2050, 2051, 2052)
    lags = [int(cases.case(f"alloc_2x{n}")[2]["n_lags"][0]) for n in cases.ALLOC_N]
    assert lags == [2045, 2047, 2049, 2049] == [cases.walk_end(n) for n in cases.ALLOC_N]
    for n in cases.ALLOC_N:
        x, kw, want = cases.case(f"alloc_2x{n}")
        assert x.shape == (2, n, 1) and want["n_draws"] == n and want["flag"].tolist() == [0]


def test_which_cases_write_rho_past_the_lds_entries():
    """The highest rho_t entry a column writes is its n_lags; it spills when that is >= 2048 (and n > 2048)."""
    for name in cases.CASES:
        _x, _kw, want = cases.case(name)
        spills = bool(want["n_draws"] > cases.RHO_LDS and want["n_lags"].max() >= cases.RHO_LDS)
        assert spills == (name in cases.SPILL), (name, want["n_lags"])
    want = cases.case("spill_2x2400")[2]
    assert want["n_lags"][[0, 2]].tolist() == [2397, 2397] and want["n_lags"][1] < 32 and want["flag"].tolist() == [0, 0, 0]
    want = cases.case("spill_global_8x2300")[2]
    assert want["n_lags"].tolist() == [2297] and want["n_chains"] * want["n_draws"] == 18400
    assert cases.case("alloc_2x2050")[2]["n_draws"] > cases.RHO_LDS          # a scratch that no entry reaches


def test_max_lag_across_the_boundary_truncates_at_or_just_below_it():
    free = cases.case("spill_2x2400")[2]
    for k in cases.SPILL_MAX_LAGS:
        want = cases.case(f"spill_max_lag_{k}")[2]
        assert want["flag"].tolist() == [4, 0, 4]
        assert want["n_lags"][[0, 2]].tolist() == [cases.max_lag_end(k)] * 2 and k - 1 <= cases.max_lag_end(k) <= k
        assert want["n_lags"][1] == free["n_lags"][1] and want["ess"][1] == free["ess"][1]
    assert [cases.max_lag_end(k) for k in cases.SPILL_MAX_LAGS] == [2047, 2047, 2049, 2099]


def test_the_monotone_pass_replaces_a_pair_on_the_boundary():
    """The second loop replaces the pair (2048, 2049) -- the first in the scratch -- by the mean of the pair (2046, 2047), the
    last in LDS, in at least one spill case; and pairs on both sides of the boundary in all that run past it."""
    on_boundary = []
    for name in ("spill_2x2400", "spill_global_8x2300", "alloc_2x2051", "alloc_2x2052"):
        _x, _kw, want = cases.case(name)
        for j, replaced in enumerate(want["replaced"]):
            if set(replaced) & {2047, 2048, 2049}:
                on_boundary.append((name, j))
    print(f"[diag-range] a replaced pair at entry 2047 - 2049: {on_boundary}")
    assert on_boundary
    replaced = cases.case("spill_2x2400")[2]["replaced"][0]
    assert min(replaced) < cases.RHO_LDS - 2 and max(replaced) > cases.RHO_LDS + 2


def test_the_checker_reports_the_replaced_pairs():
    """Every replaced pair starts at an even entry inside the walk; a column that needs the monotone pass reports some, a
    constant column none."""
    x = orc.ar1(np.random.default_rng(3), 0.0, 2, 200, 1)
    x[1] += 1.5
    c = orc.column(np.ascontiguousarray(x[:, :, 0]))
    assert c["n_lags"] == 197 and len(c["replaced"]) > 10
    assert all(k % 2 == 0 and 2 <= k <= c["n_lags"] - 3 for k in c["replaced"]) and list(c["replaced"]) == sorted(set(c["replaced"]))
    assert orc.diagnose([np.full((8, 1), 0.5)], 0.0, False)["replaced"] == [()]


# ---- B ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cases.WALK_N)
def test_walks_to_the_bound_end_on_either_side_of_a_block_edge(n):
    x, kw, want = cases.case(f"walk_2x{n}")
    assert x.shape == (2, n, 2) and want["flag"].tolist() == [0, 0]
    assert want["n_lags"].tolist() == [cases.walk_end(n)] * 2


def test_the_walks_and_stops_sit_on_both_sides_of_the_block_edges():
    assert [cases.walk_end(n) for n in cases.WALK_N] == [31, 31, 33, 33, 35, 61, 63, 63, 65, 65, 67, 93, 97]
    assert [cases.max_lag_end(k) for k in cases.EDGE_MAX_LAGS] == [29, 29, 31, 31, 33, 33, 61, 63, 63, 65, 65]
    for b in (cases.LAG_BLOCK, 2 * cases.LAG_BLOCK):
        assert {b - 1, b + 1} <= {cases.walk_end(n) for n in cases.WALK_N}
        assert {b - 1, b + 1} <= {cases.max_lag_end(k) for k in cases.EDGE_MAX_LAGS}
        assert {b - 1, b + 1} <= set(cases.RULE_STOPS)


def test_max_lag_on_block_edges_truncates_there_and_above_the_walk_changes_nothing():
    free = cases.case("edge_max_lag_398")[2]
    base = cases.dcases.case("shifted_2x400")[2]
    assert free["n_lags"].tolist() == [397] and free["flag"].tolist() == [0]
    for k in cases.FREE_MAX_LAGS:
        want = cases.case(f"edge_max_lag_{k}")[2]
        for f in orc.FIELDS + ("n_lags", "flag"):
            assert want[f].tobytes() == base[f].tobytes(), (k, f)
    for k in cases.EDGE_MAX_LAGS:
        want = cases.case(f"edge_max_lag_{k}")[2]
        assert want["flag"].tolist() == [4] and want["n_lags"].tolist() == [cases.max_lag_end(k)]


@pytest.mark.parametrize("n_lags", list(cases.RULE_STOPS))
def test_the_rule_itself_stops_a_walk_at_a_block_edge(n_lags):
    """even + odd > 0 fails at t = n_lags with the pair (t - 1, t) the last one taken, far from the n - 3 bound."""
    x, kw, want = cases.case(f"rule_stop_{n_lags}")
    assert x.shape == (2, 600, 1) and want["n_draws"] == 600
    assert want["n_lags"].tolist() == [n_lags] and want["flag"].tolist() == [0] and n_lags < 600 - 3


# ---- C ------------------------------------------------------------------------------------------------------------------
def test_the_magnitude_columns_are_what_they_are_named_for():
    for name, (seed, phi, loc, scale) in cases.MAGNITUDES.items():
        x, kw, want = cases.case(name)
        assert x.shape == (2, 600, 1) and (want["n_chains"], want["n_draws"]) == (4, 270)
        assert abs(want["mean"][0] - loc) < 0.5 * scale and 0.5 * scale < want["sd"][0] < 2 * scale
        assert want["flag"][0] == (1 if name == "scale_1e-120" else 0)
        assert np.isfinite(np.square(x)).all() and np.all(np.square(x[x != 0]) > 0)       # squares neither overflow nor vanish
    table = cases.case("magnitudes")[0]
    for j, name in enumerate(cases.MAGNITUDES):
        assert table[:, :, j].tobytes() == cases.case(name)[0][:, :, 0].tobytes()
    # the checker itself gives a column the same result next to its neighbours
    want = cases.case("magnitudes")[2]
    for j, name in enumerate(cases.MAGNITUDES):
        for f in orc.FIELDS + ("n_lags", "flag"):
            assert want[f][j:j + 1].tobytes() == cases.case(name)[2][f].tobytes(), (name, f)


def test_the_flags_at_the_constant_threshold():
    x, kw, want = cases.case("threshold")
    kept = orc.prepare(list(x), **kw)[0]
    ranges = kept.max(axis=(0, 1)) - kept.min(axis=(0, 1))
    assert ranges[:3].tolist() == list(cases.THRESHOLD_RANGES) and ranges[3] == 4 * 2.0 ** -52 == kept[:, :, 3].max() - 1.0
    assert cases.THRESHOLD_RANGES[0] < cases.THRESHOLD_RANGES[1] < 1e-15 < cases.THRESHOLD_RANGES[2]
    assert np.nextafter(cases.THRESHOLD_RANGES[1], 1.0) == 1e-15
    assert want["flag"].tolist() == list(cases.THRESHOLD_FLAGS) == [1, 1, 0, 1]
    assert want["ess"][[0, 1, 3]].tolist() == [1080.0] * 3 and np.isnan(want["rhat"][[0, 1, 3]]).all()
    assert math.isfinite(want["ess"][2]) and want["n_lags"][2] > 0


def test_scaling_by_1e_minus_7_keeps_the_order_and_the_ties_of_the_derived_columns():
    """The derived columns of the summary (ranks of x and of |x - median|, x <= q05, x <= q95) of the scale_1e-7 column are
    those of the same seed at scale 1, bit for bit: the outputs that come from them must then be equal on the device too."""
    small, unit = cases.summary_case("scale_1e-7")[2], cases.summary_case("unit")[2]
    assert cases.MAGNITUDES["scale_1e-7"][:2] == cases.MAGNITUDES["unit"][:2]
    ds, du = small["columns"][0]["derived"], unit["columns"][0]["derived"]
    for which in sorc.DERIVED + ("rank",):
        assert ds[which].tobytes() == du[which].tobytes(), which
    for k in sorc.BOUNDED:
        assert small[k].tobytes() == unit[k].tobytes(), k


@pytest.mark.parametrize("name", cases.SUMMARY_CASES)
def test_the_cases_that_go_through_the_summary_are_safe_there_too(name):
    _x, _kw, want = cases.summary_case(name)
    assert want["margin_ok"].all()
    constant = (want["flag"] & orc.FLAG_CONSTANT) != 0
    assert np.all(want["margin"][~constant] >= cases.MIN_MARGIN)


# ---- the summary's own spill ----------------------------------------------------------------------------------------------
def test_a_derived_column_of_every_spill_case_of_the_summary_walks_past_entry_2048():
    from tests import _summary_cases as scases
    for name in scases.SPILL:
        _x, _kw, want = scases.case(name)
        lags = {which: [c["parts"][which]["col"]["n_lags"] for c in want["columns"]] for which in sorc.DERIVED}
        print(f"[diag-range] summary {name}: n_lags {want['n_lags'].tolist()} derived {lags}")
        assert want["n_draws"] > cases.RHO_LDS and want["n_lags"].max() > cases.RHO_LDS
        assert max(max(v) for v in lags.values()) > cases.RHO_LDS
