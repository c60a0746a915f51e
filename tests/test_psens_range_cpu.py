"""The range cases of the PSIS weights (tests/_psens_range_cases.py) on the checker alone, without a device: every case does
what it is there for (tail counts, the ratios left above the cutoff, the sign or infinity of k, weights that underflow, the path
its size asks for), no k sits so close to 0.7 that the device's flag could go either way, the float64 checker agrees with a
50-digit evaluation of the same steps within the tolerance the device is held to, and the probe that sets that tolerance leaves
tests/_elpd_oracle as it found it."""
import math

import numpy as np
import pytest

from tests import _elpd_oracle as eorc
from tests import _psens_cases as base
from tests import _psens_oracle as orc
from tests import _psens_range_cases as rc


def test_the_case_list_is_the_one_the_range_is_made_of():
    """The tails around the workgroup's size by math.ceil, the two sizes at the LDS limit, the capacity's tail and candidates."""
    tails = {n: int(math.ceil(min(0.2 * n, 3 * math.sqrt(n)))) for n in rc.DRAW_COUNTS}
    assert (tails[7281], tails[7282], tails[7283]) == (rc.BLOCK, rc.BLOCK + 1, rc.BLOCK + 1)
    assert (tails[20], tails[21]) == (4, 5) and tails[224] == tails[225] == 45 and tails[226] == 46
    assert 0.2 * 225 == 3 * math.sqrt(225) and 0.2 * 224 < 3 * math.sqrt(224) and 0.2 * 226 > 3 * math.sqrt(226)
    assert rc.path_by_size(rc.LDS_MAX_DRAWS) == "lds" and rc.path_by_size(rc.LDS_MAX_DRAWS + 1) == "global" and 3 * math.sqrt(50_000) < 0.2 * 50_000
    assert orc.tail_count(rc.CAPACITY_DRAWS) == rc.MAX_TAIL and 30 + int(math.sqrt(rc.MAX_TAIL)) == 85 <= rc.MAX_M
    assert orc.tail_count(rc.CAPACITY_DRAWS - 1) == rc.MAX_TAIL and 30 + int(math.sqrt(orc.tail_count(50_000))) == 55
    assert len(rc.NAMES) == len(set(rc.NAMES)) and set(rc.SUMS_CASES + rc.CHAIN_CASES) <= set(rc.NAMES)
    for d in rc.DELTAS:
        for n in (25, 1000, 8000):
            assert f"delta_{d:g}_n{n}" in rc.NAMES
    assert orc.tail_count(8000) > rc.BLOCK
    three, many = rc.case("three_chains"), rc.case("sixty_four_chains")
    assert [len(c) for c in three.chains] == [40, 12, 20] and three.burn == [7, 0, 8] and three.capacity > 40 and three.piece == 3
    assert 0 not in three.columns and many.columns == [1]
    assert len(many.chains) == 64 and all(len(c) - b == 4 for c, b in zip(many.chains, many.burn)) and len(rc.stacked(many)) == 256


@pytest.mark.parametrize("name", rc.NAMES)
def test_the_case_does_what_it_is_there_for(name):
    c = rc.case(name)
    ref, vectors, expect = rc.reference(c), rc.vectors(c), c.expect
    n = len(vectors[0])
    anatomy = [orc.tail_anatomy(r) for r in vectors]
    assert len(ref.k) == 2 * len(c.columns) == len(vectors) and ref.lws.shape == (len(vectors), n)
    if "tail" in expect:
        assert all(a[0] == expect["tail"] for a in anatomy), anatomy
    if "path" in expect:
        assert expect["path"] == rc.path_by_size(n)
    for v, count in expect.get("above", {}).items():
        assert anatomy[v][1] == count, (v, anatomy[v])
    if "floored" in expect:
        assert [a[2] for a in anatomy] == expect["floored"], anatomy
    if "k_inf" in expect:
        assert np.isinf(ref.k).tolist() == expect["k_inf"], ref.k
    for v, a in enumerate(anatomy):                                          # four or fewer above the cutoff: never fitted
        assert (a[1] <= 4) <= bool(np.isinf(ref.k[v])), (v, a, ref.k[v])
    for v in expect.get("zero_weights", []):
        assert 0 < np.sum(np.exp(ref.lws[v]) == 0.0) < n - 1, v
    for v, count in expect.get("zeros", {}).items():
        assert np.sum(np.exp(ref.lws[v]) == 0.0) == count, v
    assert np.flatnonzero(ref.vflag & orc.VFLAG_CONSTANT).tolist() == expect.get("constant", [])
    for v in expect.get("k_unreliable", []):
        assert ref.k[v] > 0.7 and ref.vflag[v] == orc.VFLAG_UNRELIABLE
    # no NaN from the checker: sigma <= 0 in gpinv was not met over this grid
    assert not np.isnan(ref.lws).any() and not np.isnan(ref.k).any()
    assert np.all(np.abs(np.exp(ref.lws).sum(axis=1) - 1.0) <= 1e-12)
    # the flag cannot go either way
    finite = np.isfinite(ref.k)
    assert np.all(np.abs(ref.k[finite] - 0.7) >= 4 * ref.tol_k[finite]), (ref.k, ref.tol_k)
    assert np.all(ref.tol_k >= orc.K_TOL) and np.all(np.isfinite(ref.tol_k)) and np.all(ref.lw_spread <= 1e-11)


def test_what_some_cases_are_there_for_in_particular():
    """Five equal exceedances are fitted (k = -1.636); the tails above the workgroup are whole; delta <= 1e-4 leaves near-uniform
    weights and a k the probe moves by more than 1e-10; delta >= 0.5 gives k far above 0.7; the -inf key."""
    assert np.allclose(rc.reference(rc.case("equal_tails_25")).k[:2], -1.636, atol=1e-3)
    for n in (7282, 7283, rc.LDS_MAX_DRAWS, rc.LDS_MAX_DRAWS + 1, 50_000):
        ref, c = rc.reference(rc.case(f"draws_{n}")), rc.case(f"draws_{n}")
        assert orc.tail_anatomy(rc.vectors(c)[0])[1] > rc.BLOCK and np.isfinite(ref.k[[0, 1, 5]]).all()
    for n in (25, 1000, 8000):
        small = rc.reference(rc.case(f"delta_1e-08_n{n}"))
        assert np.all(np.abs(np.exp(small.lws) * n - 1.0) < 1e-2) and small.tol_k.max() > 100 * orc.K_TOL
        assert rc.reference(rc.case(f"delta_0.01_n{n}")).tol_k.max() < 3 * orc.K_TOL
        assert rc.reference(rc.case(f"delta_4_n{n}")).k[0] > 3.0
    assert rc.reference(rc.case("delta_1_n25")).k.max() > 15.0
    huge = rc.case("huge_entries")
    with np.errstate(over="ignore"):
        keys = [r - r.max() for r in rc.vectors(huge)]
    assert np.isfinite(keys[0]).all() and np.sum(np.isneginf(keys[1])) == 1 and np.isfinite(rc.vectors(huge)[1]).all()
    tiny = rc.reference(rc.case("tiny_ratios"))
    assert tiny.tol_k.min() > 1e-4 and np.all(tiny.lw_spread < 1e-14)
    over = rc.overflow_case()
    with np.errstate(over="ignore"):
        ratios = [s * rc.stacked(over)[:, 1] for s in orc.scales(over.delta)]
    assert np.isfinite(rc.stacked(over)).all() and np.isfinite(ratios[0]).all() and np.isinf(ratios[1]).any()


@pytest.mark.parametrize("name", [n for n in rc.NAMES if len(rc.stacked(rc.case(n))) <= 1000])
def test_the_float64_checker_against_fifty_digits(name):
    """k within the tolerance the device is held to, the log weights to 1e-10: the yardstick covers NumPy's own error."""
    c = rc.case(name)
    ref = rc.reference(c)
    for v, ratios in enumerate(rc.vectors(c)):
        if ref.vflag[v] & orc.VFLAG_CONSTANT:
            continue
        lw, k = orc.psis_weights_mp(ratios)
        assert np.isinf(k) == np.isinf(ref.k[v]) and not np.isnan(k), (v, k, ref.k[v])
        if np.isfinite(k):
            assert abs(k - ref.k[v]) <= ref.tol_k[v], (v, k, ref.k[v], ref.tol_k[v])
        assert np.array_equal(np.isneginf(lw), np.isneginf(ref.lws[v])), v
        live = np.isfinite(lw)
        assert np.allclose(ref.lws[v][live], lw[live], rtol=1e-10, atol=1e-10), (v, float(np.abs(ref.lws[v][live] - lw[live]).max()))


def test_the_probe_moves_the_last_bit_and_nothing_else():
    """k_spread is seeded and repeatable, zero for what is not fitted, grows as delta falls (the exceedances cancel), and
    tests/_elpd_oracle computes the same bits before, between and after its runs."""
    r = 0.01 * np.asarray(base.ratios(1000, 501, "normal"))
    modules = (eorc.np, eorc.math)
    before = eorc.psis_column(-r)
    first, second = orc.k_spread(r), orc.k_spread(r)
    after = eorc.psis_column(-r)
    assert (eorc.np, eorc.math) == modules and eorc.np is np and eorc.math is math
    assert first == second and 0.0 < first[0] < 1e-10 and 0.0 < first[1] < 1e-12
    assert before[0].tobytes() == after[0].tobytes() and before[1] == after[1]
    assert orc.k_spread(r, seed=7) != first and orc.tol_k(r) == orc.K_TOL + orc.K_MARGIN * first[0]
    with pytest.raises(ZeroDivisionError):                                   # the modules come back when a run fails
        with orc._jitter(0):
            1 / 0
    assert (eorc.np, eorc.math) == modules
    assert orc.k_spread(np.full(30, 2.5)) == (0.0, 0.0) and orc.k_spread(r[:20])[0] == 0.0      # constant; a tail of four
    spreads = [orc.k_spread(d * np.asarray(base.ratios(1000, 501, "normal")))[0] for d in (1e-8, 1e-6, 1e-4, 1e-2)]
    assert spreads[0] > 10 * spreads[1] > 100 * spreads[2] and spreads[2] > spreads[3]
    with orc._jitter(3):                                                     # inside: values one ulp off at the most, integers rules kept
        a = np.linspace(0.1, 5.0, 400)
        moved = eorc.np.exp(a)
        assert np.all(np.abs(moved - np.exp(a)) <= np.spacing(np.exp(a))) and np.any(moved != np.exp(a))
        assert eorc.np.sqrt(10000.0) == 100.0 and eorc.np.exp(-np.inf) == 0.0 and eorc.math.exp(-800.0) == 0.0
