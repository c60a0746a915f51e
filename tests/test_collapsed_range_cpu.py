"""The range cases of the collapsed likelihood's per-feature term (tests/_collapsed_range_cases.py) without a device: the
checker is right -- the oracle's dirichlet_categorical_logpdf (SciPy's gammaln, float64 up to the cast) meets the derived bound
on every entry of every family and equals float32(E) on every sharp entry away from a midpoint -- and it is sharp: most
entries of every family but "float32 n" are sharp by the reference alone, and three wrong restatements that the suite's older
tolerance (rtol 2e-6, atol 1e-6) accepts are rejected.  tests/test_gpu_collapsed_range.py runs the cases on the device."""
import numpy as np
import pytest
from scipy.special import gammaln

from oracle import sbayes_oracle as orc
from tests import _collapsed_range_cases as cases

F32, F64 = np.float32, np.float64


def _conc_of(c, comp, g):
    return c.conc[comp] if c.conc[comp].ndim == 2 else c.conc[comp][g]


def _oracle(c, comp):
    return np.stack([orc.dirichlet_categorical_logpdf(c.counts[comp][g], _conc_of(c, comp, g)) for g in range(c.n_groups[comp])])


@pytest.mark.parametrize("name", list(cases.CASES))
def test_the_oracle_meets_the_bound_and_is_float32_of_e_on_sharp_entries(name):
    c = cases.case(name)
    for comp in range(2):
        ref = cases.reference(name, comp)
        v = _oracle(c, comp)
        r = cases.assert_meets(ref, v, (name, comp))
        print(cases.line(f"{name} component {comp} oracle", r))
        assert ref.zero[ref.zero_counts].all() and ref.zero_counts[0, 0]               # a row without counts is exactly 0
        assert (ref.E_hi[ref.zero] == 0).all() and (ref.E_lo[ref.zero] == 0).all()
        assert (ref.E_hi[~ref.zero] < 0).all()                                         # a log-probability of at least one observation
        assert ref.k == cases.k_of(c.S) and (ref.M >= 2).all()


@pytest.mark.parametrize("family", list(cases.FAMILIES))
def test_most_entries_of_a_family_are_sharp_by_the_reference_alone(family):
    refs = [cases.reference(name, comp) for name in cases.FAMILIES[family] for comp in range(2)]
    live = sum(int((~r.zero).sum()) for r in refs)
    blunt = sum(int((~r.zero & ~r.sharp).sum()) for r in refs)
    print(f"[collapsed-range] {family}: {live} non-zero rows, {blunt} not sharp ({blunt / live:.1%}), "
          f"{sum(int(r.zero.sum()) for r in refs)} exactly zero, {sum(int((r.near_mid & r.sharp).sum()) for r in refs)} sharp within B of a midpoint")
    assert live >= 90
    if family in cases.UNCAPPED:
        return
    assert blunt <= cases.SHARP_CAP * live, (family, blunt, live)


def test_the_families_hold_what_they_are_there_for():
    assert [cases.case(n).S for n in cases.FAMILIES["S edges"]] == [1, 2, 7, 8, 9, 16, 17, 128, 129, 254]
    for name in cases.CASES:
        c = cases.case(name)
        assert c.n_groups[0] >= 1 and c.n_groups[1] >= 1 and max(c.n_groups) <= 3 and c.features.shape[0] <= 16
        assert c.conc[0].shape == (c.F, c.S) and c.conc[1].shape == (c.n_groups[1], c.F, c.S)
        for comp in range(2):
            cnt = c.counts[comp]
            assert cnt.dtype == F32 and np.array_equal(cnt, np.floor(cnt)) and (cnt >= 0).all() and cnt.max() < 2.0 ** 31
            assert (c.conc[comp].sum(axis=-1) > 0).all()
    for name, top in (("moderate", 3000), ("extreme", 60000)):
        cs = [cases.case(n) for n in cases.FAMILIES[name]]
        lo, hi = ((1e-3, 50.0), (1e-6, 1e4))[name == "extreme"]
        assert all(lo <= a.min() and a.max() <= hi for c in cs for a in c.conc)
        assert max(cnt.max() for c in cs for cnt in c.counts) > 0.9 * top
        assert min(a.min() for c in cs for a in c.conc) < 3 * lo and max(a.max() for c in cs for a in c.conc) > hi / 3
    for c in (cases.case(n) for n in cases.FAMILIES["moderate"]):
        assert {1.0, 0.5, 1.0 / c.S} <= set(np.unique(c.conc[0][1:4]).tolist())
    # masked: about 15 % of the states, a positive state in every row, counts under masked states
    for c in (cases.case(n) for n in cases.FAMILIES["masked"]):
        for comp in range(2):
            dead = np.broadcast_to(c.conc[comp] == 0, c.counts[comp].shape)
            assert 0.08 <= dead.mean() <= 0.22 and not dead.all(axis=-1).any()
            assert (c.counts[comp][dead] > 0).mean() > 0.5
    # float32 n: the float32 sum is not the integer sum
    for c in (cases.case(n) for n in cases.FAMILIES["float32 n"]):
        for comp in range(2):
            n32 = np.array([[np.sum(row, dtype=F32) for row in grp] for grp in c.counts[comp]])
            exact_n = c.counts[comp].astype(F64).sum(axis=-1)
            assert (n32 != exact_n).mean() >= 0.4 and c.counts[comp].max() >= 2.0 ** 24
    # the LDS switch of collapsed_groups(): F * S * 8 + F * 4 against 96 KB
    lds = {cases.case(n).F: cases.case(n).F * 254 * 8 + cases.case(n).F * 4 for n in cases.FAMILIES["LDS switch"]}
    assert lds[48] <= 96 * 1024 < lds[49] and all(cases.case(n).S == 254 for n in cases.FAMILIES["LDS switch"])


@pytest.mark.parametrize("s", range(1, 255))
def test_k_is_the_depth_of_numpys_pairwise_sum(s):
    """The literal recursion gives NumPy's own bits in float32 and float64, and its deepest element passes through depth(S)
    additions."""
    rng = np.random.default_rng(s)
    for dtype in (F32, F64):
        a = (rng.random(s) * 1000).astype(dtype)
        total, deepest = cases.pairwise(a)
        assert total.dtype == dtype and total.tobytes() == np.sum(a).tobytes()
        assert deepest == cases.depth(s) == cases.k_of(s) - 3
    big = np.zeros(s, dtype=F32)                                                       # the kind of row "float32 n" holds
    big[rng.integers(s)] = 2.0 ** 24
    big[rng.integers(s)] += 3
    assert cases.pairwise(big)[0].tobytes() == np.sum(big, dtype=F32).tobytes()


# ---- wrong restatements: accepted by the older tolerance, rejected by the bound ----------------------------------------------
def _restated(counts, a, wrong):
    """dirichlet_categorical_logpdf of one group, float64 up to the cast, with one of its steps done wrongly."""
    n = counts.sum(axis=-1, dtype=F32).astype(F64) if wrong != "integer n" else counts.astype(F64).sum(axis=-1)
    sum_a = a.sum(axis=-1)
    const = gammaln(sum_a) - gammaln(n + sum_a)
    y = counts.astype(F64) + a if wrong != "float32 argument" else (counts + a.astype(F32)).astype(F64)
    with np.errstate(invalid="ignore", divide="ignore"):
        series = np.where(a > 0, gammaln(y) - gammaln(a), 0.0)
    if wrong == "float32 series":
        return (const.astype(F32) + series.astype(F32).sum(axis=-1, dtype=F32)).astype(F32)
    return (const + series.sum(axis=-1)).astype(F32)


def _judged(family, wrong):
    """Per entry of the family (the exactly-zero rows included): (outside the new bound, accepted by the older tolerance
    against the oracle, not exactly zero)."""
    out, old_ok, live = [], [], []
    for name in cases.FAMILIES[family]:
        c = cases.case(name)
        for comp in range(2):
            ref = cases.reference(name, comp)
            a = np.broadcast_to(c.conc[comp], c.counts[comp].shape)
            v = np.stack([_restated(c.counts[comp][g], a[g], wrong) for g in range(c.n_groups[comp])])
            want = _oracle(c, comp)
            r = cases.check(ref, v)
            out.append((~r.within | (ref.zero & ~r.plus_zero)).ravel())
            old_ok.append((np.abs(v.astype(F64) - want) <= 1e-6 + 2e-6 * np.abs(want)).ravel())   # assert_allclose(rtol=2e-6, atol=1e-6)
            live.append(~ref.zero.ravel())
    return np.concatenate(out), np.concatenate(old_ok), np.concatenate(live)


# `floor`: the least share of the family's non-zero entries that the bound rejects (on the moderate family: and that the older
# tolerance accepts); `old_misses`: the most entries of the MODERATE family that the older tolerance may reject.  The comments
# give what was observed when the test was written.  The float32 argument is not accepted everywhere: where a is near 50 and
# the counts are 0 or 1 the spacing of float32 at c + a (3.8e-6) times digamma (4) over the states exceeds 1e-6 + 2e-6 |E| --
# 3 of 576 entries.  The integer n equals the float32 n on the moderate family (no total reaches 2^24, which is why no older
# test sees it); it is judged by the bound on the "float32 n" family.
@pytest.mark.parametrize("wrong, family, floor, old_misses", [("float32 series", "moderate", 0.50, 0),      # observed 60.6 %, 0
                                                              ("float32 argument", "moderate", 0.10, 6),    # observed 11.3 %, 3
                                                              ("integer n", "float32 n", 0.70, 0)])         # observed 83.9 %, 0
def test_the_bound_rejects_what_the_older_tolerance_accepts(wrong, family, floor, old_misses):
    assert not _judged(family, None)[0].any()                                          # the restatement itself is the oracle
    out, old_ok, live = _judged("moderate", wrong)
    print(f"[collapsed-range] {wrong} on moderate: the older tolerance rejects {int((~old_ok).sum())} of {old_ok.size} entries, "
          f"the bound {int(out.sum())}")
    assert (~old_ok).sum() <= old_misses
    if family != "moderate":                                                           # (the integer n differs where totals pass 2^24 only)
        assert not out.any()
        out, _old_ok, live = _judged(family, wrong)
        old_ok = np.ones_like(out)
    caught = out & old_ok & live
    print(f"[collapsed-range] {wrong} on {family}: {int(caught.sum())} of {int(live.sum())} non-zero entries outside the bound ({caught.sum() / live.sum():.1%})")
    assert caught.sum() >= floor * live.sum(), (wrong, int(caught.sum()), int(live.sum()))
