"""The cases of tests/_assoc_cases.py under the checker alone (tests/_assoc_oracle.py): every sweep case has the shape
and reaches the branches of Q(dof/2, statistic/2) it is meant to, few of its p-values underflow, the checker's Q agrees
with mpmath at 60 digits at every (dof, statistic) of the cases, the checker's statistic of every planted table agrees
with exact rational arithmetic, and the position and the large case are what they claim to be.  Nothing here needs a
GPU; tests/test_gpu_assoc_range.py runs the same cases on the device."""
from fractions import Fraction

import numpy as np
import pytest

from tests import _assoc_cases as ac
from tests import _assoc_oracle as ao

S_PADS = sorted(ac.SWEEP)


def _valid_pairs(r):
    v = np.triu(r["valid"], 1)
    return r["dof"][v], r["statistic"][v], r["pvalue"][v]


# ---- the sweep cases -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s_pad", S_PADS)
def test_sweep_case_has_its_shape_and_reaches_both_branches(s_pad):
    x, ns, r = ac.sweep(s_pad)
    n, f = x.shape
    assert (f, n) == ac.SWEEP[s_pad][1:] and x.dtype == np.uint8 and ns.dtype == np.int32
    # S_pad: the largest and the smallest state count that pad to it are both present
    assert ns.max() == s_pad and ns.min() == s_pad // 2 + 1
    assert np.all((x == ao.NA) | (x < ns[None, :])) and 0.02 < np.mean(x == ao.NA) < 0.04
    assert all(np.array_equal(np.unique(x[:, k][x[:, k] != ao.NA]), np.arange(ns[k])) for k in range(f))   # every state occurs
    sub, tiles, tile_pairs = ac.tiles_of(f, s_pad)
    assert (tiles, tile_pairs) == {2: (3, 6), 4: (3, 6), 8: (3, 6), 16: (4, 10), 32: (7, 28)}[s_pad]
    # the last tile is partial: fewer features than a tile edge holds, or (one feature per tile) fewer states than S_pad
    assert f % sub != 0 or (sub == 1 and ns[-1] < s_pad)
    assert n % 64 != 0 and n % ac.ROUND != 0 and n > 3 * ac.ROUND
    dof, stat, p = _valid_pairs(r)
    a, xx = 0.5 * dof, 0.5 * stat
    series = xx < np.maximum(1.0, a)
    tiny = p < ao.DBL_MIN
    print(f"S_pad {s_pad}: {len(p)} valid pairs, {int(series.sum())} on the series, {int((~series).sum())} on the fraction, "
          f"{int((p > 0.5).sum())} with p > 0.5, {int(((p < 1e-100) & ~tiny).sum())} normal below 1e-100, {int(tiny.sum())} below DBL_MIN "
          f"({int((tiny & (p > 0)).sum())} subnormal, {int((p == 0).sum())} zero), dof {dof.min()} .. {dof.max()}")
    assert series.any() and (~series).any()
    assert (p > 0.5).any() and ((p < 1e-100) & ~tiny).any()
    assert np.all((p >= 0) & (p <= 1))
    # the cap: pairs compared only as "both below DBL_MIN" are at most a quarter of the valid ones
    assert 4 * int(tiny.sum()) <= len(p)


def test_sweep_cases_together_reach_the_underflow_range_and_both_prefactors():
    dof, _stat, p = (np.concatenate(v) for v in zip(*(_valid_pairs(ac.sweep(s)[2]) for s in S_PADS)))
    assert np.any((p > 0) & (p < ao.DBL_MIN)) and np.any(p == 0)
    assert np.any(dof < 2 * ao.STIRLING_FROM) and np.any(dof > 2 * ao.STIRLING_FROM)     # the prefactor switches at a = 16
    assert len(p) == 528 + 136 + 36 + 21 + 21


# ---- the checker's Q against mpmath ------------------------------------------------------------------------------------
def _all_points():
    out = []
    for s in S_PADS:
        out.append(_valid_pairs(ac.sweep(s)[2])[:2])
    for only in (False, True):
        out.append(_valid_pairs(ac.planted(only)[3])[:2])
    dof, stat = (np.concatenate(v) for v in zip(*out))
    return dof, stat


def mp_chi2_sf(dof, stat):
    """Q(dof/2, stat/2) at 60 digits, rounded to the nearest double (subnormals and 0 included)."""
    mpmath = pytest.importorskip("mpmath")
    with mpmath.workdps(60):
        return np.array([float(mpmath.gammainc(mpmath.mpf(int(d)) / 2, mpmath.mpf(float(s)) / 2, mpmath.inf, regularized=True))
                         for d, s in zip(dof, stat)])


def test_checker_q_against_mpmath_at_every_point_of_the_cases():
    """The largest relative error over the points where the true value is a normal double is at most
    ao.GAMMA_Q_MEASURED (the figure four times of which bounds the device); below DBL_MIN the checker is below too."""
    dof, stat = _all_points()
    want = mp_chi2_sf(dof, stat)
    got = ao.chi2_sf(dof, stat)
    normal = want >= ao.DBL_MIN
    assert np.all((got[~normal] >= 0) & (got[~normal] < ao.DBL_MIN))
    assert np.all((want == 0) == (got == 0))
    rel = np.abs(got - want)[normal] / want[normal]
    worst = int(np.argmax(rel))
    print(f"checker against mpmath over {len(dof)} points ({int((~normal).sum())} below DBL_MIN): largest relative error "
          f"{rel.max():.3g} at dof {dof[normal][worst]}, statistic {stat[normal][worst]:.6g} (bound {ao.GAMMA_Q_MEASURED:.3g})")
    assert rel.max() <= ao.GAMMA_Q_MEASURED


# ---- the planted tables ------------------------------------------------------------------------------------------------
def test_exact_statistic_known_values():
    assert ac.exact_statistic(ac.PLANTED[ac.INDEPENDENT_2X2]) == (True, 1, 25, Fraction(0))
    assert ac.exact_statistic(ac.PLANTED["yates_half"]) == (True, 1, 2, Fraction(0))
    assert ac.exact_statistic(ac.PLANTED["yates_one"]) == (True, 1, 4, Fraction(1))
    assert ac.exact_statistic(ac.PLANTED["yates_clamped"]) == (True, 1, 21, Fraction(0))
    assert ac.exact_statistic(ac.PLANTED["diagonal_32"]) == (True, 961, 32, Fraction(992))
    assert ac.exact_statistic(ac.PLANTED["independent_3x3"]) == (True, 4, 36, Fraction(0))
    assert ac.exact_statistic(ac.PLANTED["never_together"]) == (False, 0, 0, Fraction(0))
    valid, dof, n, stat = ac.exact_statistic(ac.PLANTED["zero_cell"])        # [[7, 0], [3, 9]]: |E - O| = 63/19 in every cell
    assert (valid, dof, n) == (True, 1, 19)
    assert stat == sum((Fraction(63, 19) - Fraction(1, 2)) ** 2 / Fraction(r * c, 19) for r in (7, 12) for c in (10, 9))
    assert ac.exact_statistic(ac.PLANTED["ends_of_32"])[:3] == (True, 1, 25)
    assert ac.exact_statistic(ac.PLANTED["two_by_32"])[1] == 31
    assert ac.exact_statistic(np.array([[3, 4], [0, 0]]))[:3] == (False, 0, 7)


@pytest.mark.parametrize("only_2x2", [False, True])
def test_planted_tables_are_where_they_should_be_and_the_checker_is_exact_on_them(only_2x2):
    names, x, ns, r = ac.planted(only_2x2)
    f = x.shape[1]
    s = int(ns.max())
    assert s == (2 if only_2x2 else 32) and f == 2 * len(names) + 2 and x.shape[0] % 64 != 0
    assert set(names) == set(ac.PLANTED_2X2 if only_2x2 else ac.PLANTED)
    assert {"independent_2x2", "yates_half", "yates_one", "yates_clamped", "zero_cell", "never_together"} <= set(names)
    for k, name in enumerate(names):
        i, j = 2 * k, 2 * k + 1
        table = ac.planted_table(name, s)
        assert np.array_equal(r["tables"][i, j], table), name
        valid, dof, n, exact = ac.exact_statistic(table)
        assert (valid, dof, n) == (r["valid"][i, j], r["dof"][i, j], r["n"][i, j]), name
        assert ac.statistic_within(r["statistic"][i, j], table, exact), name
        got = ao.table_statistic(table)
        assert got[:3] == (valid, dof, n) and ac.statistic_within(got[3], table, exact), name
        if valid and exact == 0:
            assert r["statistic"][i, j] == 0.0 and r["pvalue"][i, j] == 1.0, name
    k = names.index("never_together")
    assert np.any(x[:, 2 * k] != ao.NA) and np.any(x[:, 2 * k + 1] != ao.NA) and r["n"][2 * k, 2 * k + 1] == 0
    assert np.all(x[:, f - 2] == ao.NA) and not r["valid"][f - 2].any() and not r["n"][f - 2].any()
    assert ns[f - 1] == 1 and np.any(x[:, f - 1] == 0) and not r["valid"][f - 1].any() and r["n"][f - 1].any()
    if not only_2x2:
        k = names.index("ends_of_32")
        assert r["dof"][2 * k, 2 * k + 1] == 1 and ns[2 * k] == 32
        k = names.index("diagonal_32")
        assert r["dof"][2 * k, 2 * k + 1] == 961 and r["statistic"][2 * k, 2 * k + 1] == 992.0


# ---- the position and the large case -----------------------------------------------------------------------------------
def test_position_case_counts():
    x, ns, want = ac.position()
    n = ac.POSITION_N
    assert x.shape == (n, n + 2) and np.all(ns == 2)
    assert np.all(np.sum(x[:, 1:n + 1] != ao.NA, axis=0) == 1) and np.all(x[np.arange(n), 1 + np.arange(n)] == 0)
    for anchor in (0, n + 1):
        assert not np.any(x[:, anchor] == ao.NA) and set(np.unique(x[:, anchor])) == {0, 1}
    r = ao.feature_association(x, ns)
    assert np.array_equal(r["n"], want)
    assert want[0, n + 1] == n and np.all(want[0, 1:n + 1] == 1) and np.all(want[n + 1, 1:n + 1] == 1) and not want[1:n + 1, 1:n + 1].any()
    assert r["valid"][0, n + 1] and int(np.triu(r["valid"], 1).sum()) == 1          # one object gives no second state
    sub, tiles, _pairs = ac.tiles_of(n + 2, 2)
    assert tiles == 33 and (n + 2) % sub != 0                                       # the anchors sit in the first and the last tile


def test_large_case_builder_at_a_small_size_and_its_exact_reference():
    """The builder at 2^16 objects (the GPU test runs it at 2^24): no NA, the planted counts, and the checker's statistic of
    the bincount tables against exact arithmetic, including the table whose cell (0, 0) is n - 520."""
    n = 1 << 16
    x, ns = ac.large(n)
    assert x.shape == (n, 6) and not np.any(x == ao.NA) and np.array_equal(ns, [2, 2, 3, 3, 32, 2]) and np.all(x < ns[None, :])
    t01 = ac.bincount_table(x, 0, 1, 2)
    assert np.array_equal(t01, [[n - 520, 220], [260, 40]])
    t23 = ac.bincount_table(x, 2, 3, 3)
    assert t23.sum() == n and n // 1000 == t23.sum() - np.trace(t23)
    want = ao.feature_association(x, ns)
    for i in range(6):
        for j in range(i + 1, 6):
            s = int(max(ns[i], ns[j]))
            table = ac.bincount_table(x, i, j, s)
            assert np.array_equal(want["tables"][i, j][:s, :s], table)
            valid, dof, cnt, exact = ac.exact_statistic(table)
            assert valid and cnt == n and dof == (ns[i] - 1) * (ns[j] - 1) == want["dof"][i, j]
            assert ac.statistic_within(want["statistic"][i, j], table, exact)
