"""The cases of tests/_clusterop_range_cases.py are what they claim to be -- shown with the log-space double alone, no GPU -- and the
double is tied to the older one (tests/_fake_engine.py, linear space) wherever that one is finite and normal.  DESIGN.md 4.3b."""
import math

import numpy as np
import pytest

from oracle import sbayes_oracle as orc
from tests import _clusterop_range_cases as cc

CS = (8, 5, 2)


def _marginal(case, tp=1.0, **kw):
    v, na = cc.marginal_v(case.st, case.probs, case.table, case.objects, tp, **kw)
    t = cc.log_terms(v)
    return v, na, t, cc.row_sums(t), cc.row_bounds(t, tempered=tp != 1.0)


def _jump(case, tp=1.0):
    v, na = cc.jump_v(case.st, case.pconf, case.p_source, case.p_target, case.objects, tp)
    t = cc.log_terms(v, skip=na)
    return v, na, t, cc.row_sums(t), cc.row_bounds(t, counted=~na, tempered=tp != 1.0)


def _range_conditions(tag, v, na, t, rows, with_na):
    finite_t = np.isfinite(t.astype(np.float64))
    n = rows.shape[1]
    below = (finite_t & (t < cc.LOG_TINY)).any(axis=-1)
    minus = np.isneginf(rows)
    one_side = minus[0] ^ minus[1]
    both = minus[0] & minus[1]
    nan = np.isnan(rows)
    counted = np.ones_like(na) if with_na else ~na
    zero_terms = int(((v == 1.0) & counted[None]).sum())
    na_nonzero = int((na[None] & finite_t & (t != 0)).sum()) if with_na else None
    print(f"[clusterop] {tag}: {2 * n} rows of {t.shape[-1]} terms: {int(below.sum())} rows hold a term below log 2^-126 (smallest "
          f"{float(t[finite_t].min()):.1f}), {int(one_side.sum())} rows -inf on one side only, {int(both.sum())} objects -inf on both, "
          f"{int(nan.sum())} NaN rows, {zero_terms} terms exactly 0, NA terms not 0: {na_nonzero}, non-finite rows {int((~np.isfinite(rows)).sum())}")
    assert below.sum() >= 20
    assert (below & np.isfinite(rows)).sum() >= 20              # ... in rows that are held to their bound
    assert one_side.sum() >= 10 and both.sum() >= 3 and nan.sum() >= 1
    assert zero_terms >= 20
    if with_na:
        assert na_nonzero >= 50
    assert (~np.isfinite(rows)).sum() <= rows.size // 2
    assert not np.isposinf(rows).any() and not (v > 1.0 + 1e-6).any()


@pytest.mark.parametrize("C", CS)
def test_marginals_cases_reach_the_range(C):
    case = cc.value_case(C)
    assert case.st.shape[0] <= 70
    objs = case.objects
    assert (np.diff(objs) < 0).any() and np.unique(objs).size == objs.size - 1              # unsorted, one object twice
    assert (~case.st.has_components[:, 1:].any(axis=1)).sum() == 3                           # objects outside every confounder group
    for name, tab in (("candidate", case.table), *((f"component {c}", case.probs[c]) for c in range(1, C))):
        for value in (0.0, cc.DENORMAL, cc.TINY, 1.0):
            assert (tab == cc.F32(value)).any(), (name, value)
    w = cc.weights_z(case.st)
    assert (w == 0).any() and ((w > 0) & (w < cc.TINY)).any() and np.isnan(w).any()
    v, na, t, rows, _ = _marginal(case)
    _range_conditions(f"marginals C={C}", v, na, t, rows, with_na=True)
    i, j = np.flatnonzero(objs == objs[3])[:2]
    assert np.array_equal(rows[:, i], rows[:, j], equal_nan=True)                            # the repeated object: the same two rows


@pytest.mark.parametrize("C", CS)
def test_jump_cases_reach_the_range(C):
    case = cc.value_case(C)
    for name, tab in (("source", case.p_source), ("target", case.p_target), ("confounders", case.pconf)):
        for value in (0.0, cc.DENORMAL, cc.TINY, 1.0):
            assert (tab == cc.F32(value)).any(), (name, value)
    v, na, t, rows, _ = _jump(case)
    _range_conditions(f"jump C={C}", v, na, t, rows, with_na=False)
    assert (t[:, na] == 0).all()                                                             # NA is skipped: no term


@pytest.mark.parametrize("C", CS)
def test_the_bound_sees_dropped_na_terms_and_swapped_sides(C):
    """A kernel that skipped NA features (right for the jump, wrong for the marginals: the term is log sum_c w_c), and one that took
    the other side's weight row, each move at least one row by more than 100 bounds."""
    case = cc.value_case(C)
    _, _, _, rows, bound = _marginal(case)
    fin = np.isfinite(rows)
    v, _ = cc.marginal_v(case.st, case.probs, case.table, case.objects, drop_na=True)
    dropped = cc.row_sums(cc.log_terms(v))
    both = fin & np.isfinite(dropped)
    dropped = np.where(both, dropped, 0.0)
    rows = np.where(fin, rows, 0.0)
    ratio = np.abs(dropped - rows)[both] / bound[both]
    print(f"[clusterop] C={C}: NA terms dropped: largest move {ratio.max():.3g} bounds ({np.abs(dropped - rows)[both].max():.3e})")
    assert ratio.max() > 100
    v, _ = cc.marginal_v(case.st, case.probs, case.table, case.objects, wz=cc.weights_z(case.st)[::-1])
    swapped = cc.row_sums(cc.log_terms(v))
    both = fin & np.isfinite(swapped)
    swapped = np.where(both, swapped, 0.0)
    ratio = np.abs(swapped - rows)[both] / bound[both]
    print(f"[clusterop] C={C}: sides' weight rows swapped: largest move {ratio.max():.3g} bounds")
    assert ratio.max() > 100
    # one float32 ulp in one weight of one feature is seen too, wherever that feature's term is not tiny against the row's bound
    w = cc.weights_z(case.st).copy()
    n = int(case.objects[0])
    f = int(np.flatnonzero(~case.st.na[n])[0])
    c = int(np.nanargmax(w[1, n, f]))
    w[1, n, f, c] = np.nextafter(w[1, n, f, c], cc.F32(0))
    v, _ = cc.marginal_v(case.st, case.probs, case.table, case.objects[:1], wz=w)
    moved = cc.row_sums(cc.log_terms(v))[1, 0]
    if math.isfinite(rows[1, 0]):
        print(f"[clusterop] C={C}: one weight one float32 ulp down: row moves {abs(moved - rows[1, 0]):.3e}, bound {bound[1, 0]:.3e}")


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("tp", [1.5, 1.7])
def test_tempered_zero_pattern(C, tp):
    """powf keeps 0 at 0 and a positive normalised weight positive: the zero / -inf / NaN pattern of every term and row is the
    untempered one.  (Not so the weights' own: 1e-30 u beside 1e30 normalises to exactly 0, but tempered BEFORE it is normalised --
    the flipped side -- to a denormal; such a weight meets no v that is 0 without it.)"""
    case = cc.value_case(C)
    for f in (_marginal, _jump):
        _, _, t1, rows1, _ = f(case)
        _, _, t, rows, bound = f(case, tp)
        assert np.array_equal(cc.pattern(t), cc.pattern(t1)) and np.array_equal(cc.pattern(rows), cc.pattern(rows1))
        assert (bound >= cc.POWF).all()
    w1, w = cc.weights_z(case.st), cc.weights_z(case.st, tp)
    assert np.array_equal(np.isnan(w), np.isnan(w1)) and (w[w1 > 0] > 0).all() and (np.nan_to_num(w[:, :, case.st.weights == 0]) == 0).all()


def _fake_pair(st):
    fake = cc.double_of(st)
    probs = [None] + [orc.component_probs(st.counts[c], st.conc[c]) for c in range(1, len(st.groups))]
    return fake, probs


@pytest.mark.parametrize("name", ["f63", "f64", "f255", "f257", "c1", "range8", "range5", "range2"])
@pytest.mark.parametrize("tp", [1.0, 1.5])
def test_agrees_with_the_linear_space_double(name, tp):
    """Where FakeEngine's linear-space value (np.prod, then a log; einsum over the components) is finite and normal, the log-space
    double agrees with it to 1e-9 -- marginals and jump, on ordinary states and on the range states whose rows never sum to 0."""
    st = cc.range_state(int(name[5:])) if name.startswith("range") else cc.edge_state(name)
    fake, probs = _fake_pair(st)
    N, F, C = st.shape
    K = st.groups[0].shape[0]
    objs = np.arange(N)                                               # (FakeEngine takes a mask: ascending, no repeats)
    table = orc.component_probs(st.counts[0][[0]], st.conc[0])[0]
    with np.errstate(under="ignore", invalid="ignore", divide="ignore"):
        old = fake.cluster_marginals(0, table, objs, tp)
    new = cc.row_sums(cc.log_terms(cc.marginal_v(st, probs, table, objs, tp)[0]))
    ok = np.isfinite(old) & (old > math.log(np.finfo(np.float64).tiny))
    assert ok.sum() >= min(N, 20) or F > 200, (name, int(ok.sum()))
    if ok.any():
        np.testing.assert_allclose(new[ok], old[ok], rtol=1e-9, atol=1e-9)
    if C > 1:
        assert np.array_equal(np.isnan(new), np.isnan(old))
    # jump: FakeEngine.jump_lh already sums logs, of oracle values: the float32 chain is the oracle's bit for bit
    pconf = np.concatenate(probs[1:]) if C > 1 else np.zeros((0, F, st.features.shape[2]), dtype=cc.F32)
    p_tgt = orc.component_probs(st.counts[0][[1 % K]], st.conc[0])[0]
    v, na = cc.jump_v(st, pconf, table, p_tgt, objs, tp)
    new = cc.row_sums(cc.log_terms(v, skip=na))
    old = fake.jump_lh(0, pconf, table, p_tgt, objs, tp)
    fin = np.isfinite(old)
    assert np.array_equal(np.isfinite(new), fin) and fin.any()
    np.testing.assert_allclose(new[fin], old[fin], rtol=1e-9, atol=1e-9)
    if tp == 1.0:
        members = st.groups[0][0]
        stay, jump = orc.jump_lh_per_feature(st.features, st.groups, st.counts, st.conc, st.unif, st.weights, 0, 1 % K)
        mine, _ = cc.jump_v(st, pconf, orc.conditional_effect_mean(st.conc[0], st.counts[0][[0]], st.unif, 1.0, 1.0)[0],
                            orc.conditional_effect_mean(st.conc[0], st.counts[0][[1 % K]], st.unif, 1.0, 1.0)[0],
                            np.flatnonzero(members))
        seen = ~st.na[members]
        assert np.array_equal(mine[0][seen].astype(cc.F32), stay[seen]) and np.array_equal(mine[1][seen].astype(cc.F32), jump[seen])


def test_edge_and_limit_cases_are_what_they_claim():
    assert sorted(st_shape[1] for st_shape in cc.EDGE_SHAPES.values())[:8] == [1, 20, 63, 64, 65, 255, 256, 257]
    assert {len(s[4]) + 2 for s in cc.EDGE_SHAPES.values()} | {1} == {1, 3, 4, 5, 8}
    assert {s[2] for s in cc.EDGE_SHAPES.values()} >= {16, 17, 33}
    assert cc.additions(513) == 11 and cc.additions(256) == 9 and cc.additions(1) == 9
    for name in (*cc.EDGE_SHAPES, "c1"):
        st = cc.edge_state(name)
        i_source, i_target, lists = cc.member_lists(st, 1)
        assert all(st.groups[0][i_source][lists[n]].all() and lists[n].size == n for n in cc.SIZES)
        assert all(v.size == n for n, v in cc.available_lists(st, i_source, 2).items())
    want = {"marginals-512": 65536, "marginals-513": 65664, "jump-7-7": 65536, "jump-7-8": 69632}
    for name, size in want.items():
        st, table_bytes = cc.limit_state(name)
        assert table_bytes == size and len(st.groups) <= 4, (name, table_bytes)
        assert (table_bytes <= cc.LIMIT_BYTES) == name.endswith(("512", "7-7"))
        assert name.startswith("marginals") or st.groups[0].sum(axis=1).max() >= 3


def test_source_lh_cases():
    st = cc.slf_entry_state()
    p = cc.slf_selected(st)[0]
    assert st.shape == (1, cc.SLF_F, 2) and (p > 0).all()
    assert ((p > 0) & (p < cc.TINY)).sum() >= 50 and (p == 1).sum() >= 50 and ((p > 0.25) & (p < 1)).sum() >= 100
    assert p.min() == 2.0 ** -149 and np.unique(p).size > cc.SLF_F // 3
    for N, F in cc.SLF_EDGES:
        st = cc.slf_edge_state(N, F)
        sel = cc.slf_selected(st)
        want, bound = cc.slf_double(st)
        assert st.shape[:2] == (N, F)
        assert want[0] == -math.inf and want[F - 1] == -math.inf and want[1] == 0.0 and bound[1] == 0.5 * float(cc.ulp32(0.0))
        assert (sel[:, 0] == 0).any() and st.na[:, 1].all() and not st.na[N - 1, F - 1] and st.source_ids[N - 1, F - 1] == 255
        mid = np.isfinite(want) & (want != 0)
        assert mid.sum() == F - 3 and (bound[mid] < 1e-4 * np.abs(want[mid])).all()
        # the double is the oracle's value to float32 accuracy
        w = orc.normalize_weights(st.weights, st.has_components)
        old = orc.source_lh_by_feature(st.source, w, st.na)
        np.testing.assert_allclose(old[mid], want[mid], rtol=1e-4)
