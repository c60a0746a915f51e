"""The feature screening on the device (sbayes_amd.assoc, csrc/sbe_assoc.hip) over its state, object and p-value range,
on the seeded cases of tests/_assoc_cases.py (tests/test_assoc_cases_cpu.py proves under the checker alone that they
cover what they claim): every padded state count including S_pad = 4, planted tables at the exact corners of Yates'
correction against rational arithmetic, the p-value at the device's own statistic against the checker and against
mpmath, bit-identical results under any order of the objects, every position of the FP4 operand, and 2^24 objects
(the documented limit: a count above 2^24 - 1000 in the f32 accumulator, two launches under the default chunking)."""
import numpy as np
import pytest

from sbayes_amd import assoc
from tests import _assoc_cases as ac
from tests import _assoc_oracle as ao
from tests.test_gpu_assoc import _against_oracle, _same_bits

pytestmark = pytest.mark.gpu

S_PADS = sorted(ac.SWEEP)
DOF_BUCKETS = [(1, 1), (2, 15), (16, 31), (32, 63), (64, 255), (256, 961)]      # (a = dof / 2: the prefactor switches at dof 32)


def _mp_chi2_sf(dof, stat):
    """Q(dof/2, stat/2) at 60 digits rounded to double, or None without mpmath."""
    try:
        import mpmath
    except ImportError:
        return None
    with mpmath.workdps(60):
        return np.array([float(mpmath.gammainc(mpmath.mpf(int(d)) / 2, mpmath.mpf(float(s)) / 2, mpmath.inf, regularized=True))
                         for d, s in zip(dof, stat)])


def _pvalue_at_own_statistic(label, dof, stat, pv):
    """Every valid p-value lies in [0, 1] and is within ao.PVALUE_BOUND (relative) of Q(dof/2, statistic/2) at the device's
    own statistic, by the checker and (where importable) by mpmath; where the reference is below DBL_MIN, 0 <= p < DBL_MIN."""
    dof, stat, pv = np.asarray(dof), np.asarray(stat), np.asarray(pv)
    assert np.all((pv >= 0) & (pv <= 1)), label
    for ref_name, ref in (("checker", ao.chi2_sf(dof, stat)), ("mpmath", _mp_chi2_sf(dof, stat))):
        if ref is None:
            print(f"{label}: mpmath is not importable, the p-value is compared with the checker only")
            continue
        tiny = ref < ao.DBL_MIN
        rel = np.zeros(len(pv))
        rel[~tiny] = np.abs(pv - ref)[~tiny] / ref[~tiny]
        parts = []
        for lo, hi in DOF_BUCKETS:
            m = (dof >= lo) & (dof <= hi) & ~tiny
            if m.any():
                parts.append(f"dof {lo}-{hi}: {rel[m].max():.3g} ({int(m.sum())})")
        print(f"{label}: p-value against {ref_name} at the device's statistic, largest relative error {rel.max():.3g} "
              f"(bound {ao.PVALUE_BOUND:.3g}), {int(tiny.sum())} below DBL_MIN; " + ", ".join(parts))
        assert np.all((pv[tiny] >= 0) & (pv[tiny] < ao.DBL_MIN)), (label, ref_name)
        assert np.all(rel <= ao.PVALUE_BOUND), (label, ref_name)


def _upper_pairs(f):
    return np.argwhere(np.triu(np.ones((f, f), dtype=bool), 1))


def _check_case(label, x, ns, r, s_pad):
    """The rules every sweep and planted case is held to; returns the device's result."""
    res = assoc.feature_association(x, ns)
    f = x.shape[1]
    assert assoc.handle_for(0).last_shape()[:2] == (s_pad, ac.tiles_of(f, s_pad)[2])
    _against_oracle(res, r, label)                           # integers equal, symmetric, statistic and p-value at their bounds
    assert np.array_equal(res.pvalue, res.pvalue.T, equal_nan=True)
    v = np.triu(res.valid, 1)
    _pvalue_at_own_statistic(label, res.dof[v], res.statistic[v], res.pvalue[v])
    pairs = _upper_pairs(f)                                  # the table kernel: every pair, against the checker's tables
    s = int(ns.max())
    tabs = res.tables(pairs)
    assert tabs.shape == (len(pairs), s, s) and np.array_equal(tabs, r["tables"][pairs[:, 0], pairs[:, 1]])
    return res


@pytest.mark.parametrize("s_pad", S_PADS)
def test_sweep_case_against_the_checker(s_pad):
    x, ns, r = ac.sweep(s_pad)
    _check_case(f"sweep S_pad {s_pad}", x, ns, r, s_pad)


@pytest.mark.parametrize("only_2x2", [False, True])
def test_planted_tables_against_exact_arithmetic(only_2x2):
    """Pair (2 k, 2 k + 1) holds a table whose statistic is known in rational arithmetic: the device is within
    ao.statistic_bound(R, C) exact + n 2^-100 of it, and returns statistic 0.0 and p-value 1.0 bit for bit where the
    exact statistic is 0 (E = O in every cell, or Yates' correction removes the whole difference)."""
    names, x, ns, r = ac.planted(only_2x2)
    s_pad = 2 if only_2x2 else 32
    res = _check_case(f"planted S_pad {s_pad}", x, ns, r, s_pad)
    s = int(ns.max())
    tabs = res.tables([(2 * k, 2 * k + 1) for k in range(len(names))])
    for k, name in enumerate(names):
        i, j = 2 * k, 2 * k + 1
        table = ac.planted_table(name, s)
        assert np.array_equal(tabs[k], table), name
        valid, dof, n, exact = ac.exact_statistic(table)
        assert (valid, dof, n) == (res.valid[i, j], res.dof[i, j], res.n[i, j]), name
        assert ac.statistic_within(res.statistic[i, j], table, exact), (name, res.statistic[i, j], float(exact))
        if valid and (exact == 0 or name == ac.INDEPENDENT_2X2):
            assert res.statistic[i, j].tobytes() == np.float64(0.0).tobytes(), name
            assert res.pvalue[i, j].tobytes() == np.float64(1.0).tobytes(), name
        if not valid:
            assert res.statistic[i, j] == 0 and np.isnan(res.pvalue[i, j]) and res.dof[i, j] == 0, name
    if not only_2x2:
        k = names.index("diagonal_32")
        assert res.dof[2 * k, 2 * k + 1] == 961 and res.statistic[2 * k, 2 * k + 1] == 992.0
        k = names.index("ends_of_32")
        assert res.dof[2 * k, 2 * k + 1] == 1
    k = names.index("yates_one")
    assert res.statistic[2 * k, 2 * k + 1] == 1.0


# ---- the order of the objects ------------------------------------------------------------------------------------------
def test_object_order_changes_no_bit():
    """Rotating the objects moves every one of them to another (lane half, dword, nibble) of the FP4 operand and, from 64
    on, to another contraction step; the counts are integers, so all five outputs keep every bit."""
    x, ns, _r = ac.sweep(8)
    base = assoc.feature_association(x, ns)
    for shift in (1, 31, 32, 33, 64, 255):
        assert _same_bits(base, assoc.feature_association(np.roll(x, shift, axis=0), ns)), shift
    perm = np.random.default_rng(8).permutation(x.shape[0])
    assert _same_bits(base, assoc.feature_association(x[perm], ns))


def test_every_operand_position_counts_once():
    x, ns, want = ac.position()
    res = assoc.feature_association(x, ns)
    assert assoc.handle_for(0).last_shape()[:2] == (2, 33 * 34 // 2)
    assert np.array_equal(res.n, want)
    r = ao.feature_association(x, ns)
    _against_oracle(res, r, "position")
    assert int(np.triu(res.valid, 1).sum()) == 1 and res.valid[0, ac.POSITION_N + 1]


# ---- 2^24 objects ------------------------------------------------------------------------------------------------------
def test_counts_are_exact_at_the_object_limit():
    """2^24 objects without NA: every n is 2^24, the table of the two sparse binary features has a cell of 2^24 - 520 (the
    f32 accumulator adds 0/1 products exactly up to there, which include/sbe_assoc.h promises), and the default chunking
    splits both kernels' work into two launches (21 tile pairs, 16 per launch; 21 tables likewise)."""
    n = ac.LARGE_N
    x, ns = ac.large()
    h = assoc.handle_for(0)
    h._data = None                                             # (the device's codes belong to no result object from here on)
    statistic, pvalue, dof, cnt, valid = h.compute(x, ns)      # (directly: the Python layer's checks make int64 temporaries)
    assert h.last_shape() == (32, 21, 2)
    print(f"2^24 objects: pair kernel {h.last_kernel_ms():.1f} ms over two launches")
    pairs = _upper_pairs(6)
    asked = np.concatenate([pairs, pairs[:6, ::-1]])           # 21 tables: two launches of the table kernel as well
    tabs = h.tables(asked, 32)
    for out in (statistic, dof, cnt, valid):
        assert np.array_equal(out, out.T)
    assert np.array_equal(pvalue, pvalue.T, equal_nan=True)
    assert not valid.diagonal().any() and np.all(np.isnan(pvalue.diagonal())) and not cnt.diagonal().any()
    dofs, stats, pvs = [], [], []
    for k, (i, j) in enumerate(pairs):
        table = ac.bincount_table(x, i, j, 32)
        assert np.array_equal(tabs[k], table), (i, j)
        if k < 6:
            assert np.array_equal(tabs[len(pairs) + k], table.T), (j, i)
        want_valid, want_dof, want_n, exact = ac.exact_statistic(table)
        assert want_n == n and want_valid and want_dof == (ns[i] - 1) * (ns[j] - 1)
        assert (cnt[i, j], dof[i, j], bool(valid[i, j])) == (n, want_dof, True), (i, j)
        assert ac.statistic_within(statistic[i, j], table, exact), (i, j, statistic[i, j], float(exact))
        dofs.append(dof[i, j]), stats.append(statistic[i, j]), pvs.append(pvalue[i, j])
    assert tabs[0][0, 0] == n - 520 and tabs[0][0, 0] > n - 1000
    _pvalue_at_own_statistic("2^24 objects", dofs, stats, pvs)
