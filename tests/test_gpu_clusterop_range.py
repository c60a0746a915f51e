"""The cluster operators' marginals and jump scores over their range: k_cluster_marginals / k_cluster_marginals_ws, k_jump_lh /
k_jump_lh_ws and k_source_lh_by_feature (sbayes_amd/csrc/sbe_kernels_operators.hip.h) against the log-space double of
tests/_clusterop_range_cases.py -- tests/test_clusterop_range_cpu.py proves with the double alone that the cases are what they
claim to be.  DESIGN.md section 4.3b.

At T_prior = 1 the device's v of every (object, side, feature) is the double's bit for bit (no contraction in the build); the
table log and the order of the sum differ, so a finite row is held to
    |device - double| <= sum_f 1.5 (ulp(|t_f|) + 2^-53) + D 2^-53 sum_f |t_f|,      D = ceil(F / 256) + 8,
a row the double has at -inf or NaN is -inf or NaN on the device, the other side of that object is still held to its bound, and
no error is raised.  Tempered, 2e-6 per feature is added (float32 powf).  On every case the fused form equals the block form
and the resident form equals the explicit-table form fed with normalize_tables' tables, bit for bit.  Every test prints
`[clusterop]` lines: rows compared and the largest error / bound.

Which test fails under which change of the kernels (reasoned from the code, not run):
    NA features skipped in the marginals   every marginals test: the NA term is log sum_c w_c, 1e-7 or so, against bounds of 1e-13
                                           (CPU-asserted: > 100 bounds)
    `inside ? a : b` swapped, or a / b     every marginals test (> 1e13 bounds), and the -inf rows change sides
    lh of a missing group not 0            test_value_range_*: objects outside confounder groups
    tab_log_pos's special path not taken   test_value_range_*: v = 0 must give -inf, NaN NaN; tab_log_core returns a finite number
    `c < C` dropped in the v loops         C < 8 in the block form, C < 4 in the fused form: wc / wf behind C are 0 and lh 1: no
                                           change of any result (the guard is implied)
    a pass of the ws forms out of order    test_shape_edges[f257, f513], test_fused_limit: fused != block bit for bit
"""
import math

import numpy as np
import pytest

from sbayes_amd.engine import Engine
from tests import _clusterop_range_cases as cc

pytestmark = pytest.mark.gpu

F32 = np.float32
LOGF_ULPS = 2.5                                  # the device logf against the float32-rounded exact log: observed 2, plus 1/2


def _engine(st):
    return cc.load(Engine(st.features, st.n_groups, n_slots=1), st)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(nan, np.isnan(b)) and \
        np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


def _hold(tag, got, t, counted=None, tempered=False):
    """Device rows [2, n] against the double's terms t [2, n, F]: the -inf / NaN pattern equal, every finite row within its bound."""
    want, bound = cc.row_sums(t), cc.row_bounds(t, counted, tempered)
    assert got.shape == want.shape and got.dtype == np.float64, (tag, got.shape, got.dtype)
    pat = cc.pattern(want)
    fin = pat == 0
    err = np.abs(np.where(fin, got, 0.0) - np.where(fin, want, 0.0))
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(fin, err / bound, -1.0)
    j = np.unravel_index(int(ratio.argmax()), ratio.shape)
    print(f"[clusterop] {tag}: {int(fin.sum())} finite rows of {t.shape[-1]} terms, largest error / bound {ratio[j]:.3f} (error {err[j]:.3e}, "
          f"bound {bound[j]:.3e}, row {want[j]:.6g}), largest error {err.max():.3e}; {int((pat == 1).sum())} rows -inf, {int((pat == 2).sum())} NaN")
    assert np.array_equal(cc.pattern(got), pat), (tag, "special rows", np.argwhere(cc.pattern(got) != pat)[:8].tolist())
    assert (err <= np.where(fin, bound, 0.0)).all(), (tag, j, float(got[j]), float(want[j]), float(err[j]), float(bound[j]))
    return float(ratio[j]), float(err.max())


def _forms(eng, call):
    """The resident call fused and not: bit-equal.  -> the fused result."""
    eng.set_option(fuse_tables=True)
    a = call()
    eng.set_option(fuse_tables=False)
    b = call()
    eng.set_option(fuse_tables=True)
    return a, b


def _tables(eng, st, groups, c, t, tp):
    """normalize_tables of rows `groups` of component c, tempered with the CLUSTER prior's uniform concentration like the operators."""
    conc = st.conc[c] if c == 0 else st.conc[c][groups]
    return eng.normalize_tables(st.counts[c][groups], conc, temperature=t, prior_temperature=tp, unif_counts=st.unif)


def _resident_marginals(eng, st, k, objs, t=1.0, tp=1.0, tag=""):
    tag = f"{st.name} marginals resident n={len(objs)} T={t} Tp={tp} {tag}"
    fused, block = _forms(eng, lambda: eng.cluster_posterior_marginals(0, k, objs, t, tp))
    assert _same_bits(fused, block), (tag, "fused != block")
    table = _tables(eng, st, [k], 0, t, tp)[0]
    assert _same_bits(eng.cluster_marginals(0, table, objs, tp), fused), (tag, "resident != explicit tables")
    probs = [None] + [eng.get_probs(0, c) for c in range(1, len(st.groups))]
    v, _ = cc.marginal_v(st, probs, table, objs, tp)
    return _hold(tag, fused, cc.log_terms(v), tempered=tp != 1.0)


def _resident_jump(eng, st, i_source, i_target, objs, t=1.0, tp=1.0, tag=""):
    tag = f"{st.name} jump resident n={len(objs)} T={t} Tp={tp} {tag}"
    C = len(st.groups)
    fused, block = _forms(eng, lambda: eng.jump_lh_resident(0, i_source, i_target, objs, t, tp))
    assert _same_bits(fused, block), (tag, "fused != block")
    ps, pt = _tables(eng, st, [i_source], 0, t, tp)[0], _tables(eng, st, [i_target], 0, t, tp)[0]
    F, S = ps.shape
    pconf = np.concatenate([_tables(eng, st, slice(None), c, t, tp) for c in range(1, C)]) if C > 1 else np.zeros((0, F, S), dtype=F32)
    assert _same_bits(eng.jump_lh(0, pconf, ps, pt, objs, tp), fused), (tag, "resident != explicit tables")
    v, na = cc.jump_v(st, pconf, ps, pt, objs, tp)
    return _hold(tag, fused, cc.log_terms(v, skip=na), counted=~na, tempered=tp != 1.0)


# ---- 1: the value range, explicit-table forms ----------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [8, 5, 2])
def test_value_range_marginals(C):
    """Weights of exactly 0, 1e-42, 2^-126 and 1e30 beside 1e-30, a weight row of exactly (0, 1, 0, ..), weight rows that sum to 0;
    candidate and confounder entries of exactly 0, 1e-42, 2^-126 and 1; objects outside every confounder group; NA; an unsorted
    list with one object twice: rows of -inf on one side, on both, NaN rows, terms below log 2^-126 and terms of exactly 0."""
    case = cc.value_case(C)
    st = case.st
    eng = _engine(st)
    try:
        for t, tp in ((1.0, 1.0), *cc.TEMPERATURES):               # the slot's own tables (zeros and denormals of the tiny concentrations)
            _resident_marginals(eng, st, 0, case.objects, t, tp)
        for c in range(1, C):
            eng.set_probs(0, c, case.probs[c])
        for tp in (1.0, 1.5, 1.7):
            got = eng.cluster_marginals(0, case.table, case.objects, tp)
            v, _ = cc.marginal_v(st, case.probs, case.table, case.objects, tp)
            _hold(f"value{C} marginals planted Tp={tp}", got, cc.log_terms(v), tempered=tp != 1.0)
            if tp == 1.0:
                i, j = np.flatnonzero(case.objects == case.objects[3])[:2]
                assert _same_bits(got[:, i], got[:, j])             # the object listed twice
        _resident_marginals(eng, st, 1, case.objects, tag="planted confounder tables")
    finally:
        eng.close()


@pytest.mark.parametrize("C", [8, 5, 2])
def test_value_range_jump(C):
    """The same states through ClusterJump's scores: source, target and confounder entries of exactly 0, 1e-42, 2^-126 and 1."""
    case = cc.value_case(C)
    st = case.st
    eng = _engine(st)
    try:
        for tp in (1.0, 1.5, 1.7):
            got = eng.jump_lh(0, case.pconf, case.p_source, case.p_target, case.objects, tp)
            v, na = cc.jump_v(st, case.pconf, case.p_source, case.p_target, case.objects, tp)
            _hold(f"value{C} jump planted Tp={tp}", got, cc.log_terms(v, skip=na), counted=~na, tempered=tp != 1.0)
        for t, tp in ((1.0, 1.0), *cc.TEMPERATURES):
            _resident_jump(eng, st, 0, 1, case.objects, t, tp)
    finally:
        eng.close()


# ---- 2: shape edges, ordinary states, both forms -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [*cc.EDGE_SHAPES, "c1"])
def test_shape_edges(name):
    """F = 1, 63, 64, 65, 255, 256, 257, 513 (513: the third pass holds one feature), n_av and n_members = 1, 3, 4, 5, 9 (four object
    waves per wave-specialised block), C = 1, 3, 4 (fused), 5, 8 (block form only), S = 16, 17, 33; lists unsorted."""
    st = cc.edge_state(name)
    eng = _engine(st)
    try:
        i_source, i_target, members = cc.member_lists(st, 60)
        available = cc.available_lists(st, i_source, 61)
        for n in cc.SIZES:
            _resident_marginals(eng, st, i_source, available[n])
            _resident_jump(eng, st, i_source, i_target, members[n])
        _resident_marginals(eng, st, i_source, available[5], 1.3, 1.5)
        _resident_jump(eng, st, i_source, i_target, members[5], 1.3, 1.5)
    finally:
        eng.close()


# ---- 3: the fused forms' table limit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cc.LIMITS))
def test_fused_limit(name):
    """Tables of exactly 64 KB (fused: with the 2 KB log table the block holds 66 KB of LDS) and just beyond (table kernels in
    front): both answer, alike with the option off, and within the bound."""
    st, table_bytes = cc.limit_state(name)
    eng = _engine(st)
    try:
        N = st.shape[0]
        if cc.LIMITS[name][0] == "marginals":
            _resident_marginals(eng, st, 0, np.random.default_rng(70).permutation(N).astype(np.int32), tag=f"{table_bytes} B")
        else:
            i_source = int(st.groups[0].sum(axis=1).argmax())
            members = np.flatnonzero(st.groups[0][i_source])[::-1].astype(np.int32)
            _resident_jump(eng, st, i_source, 1 - i_source, members, tag=f"{table_bytes} B")
    finally:
        eng.close()


# ---- 4: k_source_lh_by_feature -------------------------------------------------------------------------------------------------------------
def test_source_lh_entry_by_entry():
    """N = 1: out[f] is logf of one normalised weight, from 2^-149 to 1.  The device library's logf is NOT within 1 float32 ulp of
    the float32-rounded exact log: measured on the MI355X over these 4000 weights, 73 % bit-equal, the largest distance 2 ulp
    (at w = 0x1.818814p-86, log w = -59.2: the error grows with |log w|).  The bound is that observation plus half an ulp
    (DESIGN.md 4.3b)."""
    st = cc.slf_entry_state()
    eng = _engine(st)
    try:
        got = eng.source_lh_by_feature(0)
    finally:
        eng.close()
    p = cc.slf_selected(st)[0]
    want = np.log(p.astype(np.longdouble)).astype(F32)
    assert got.dtype == F32 and got.shape == want.shape
    ulps = np.abs(got.astype(np.float64) - want.astype(np.float64)) / cc.ulp32(want)
    ulps[(want == 0) & (got == 0)] = 0.0
    j = int(ulps.argmax())
    print(f"[clusterop] logf over {p.size} normalised weights from {p.min():.3e} to {p.max()}: largest distance from the float32-rounded "
          f"exact log {ulps[j]:.3f} ulp (w = {float(p[j]).hex()}), {int((ulps == 0).sum())} bit-equal")
    assert ulps[j] <= LOGF_ULPS, (ulps[j], float(p[j]).hex(), got[j], want[j])
    assert (got[p == 1] == 0).all()


@pytest.mark.parametrize("N,F", cc.SLF_EDGES)
def test_source_lh_edges(N, F):
    """N = 511, 512, 513 (a pass is 64 lanes x 8 objects), F = 15, 16, 17 (a block is 16 features): a zero weight at a source and an
    observation without a source give -inf, a feature that is NA throughout exactly 0."""
    st = cc.slf_edge_state(N, F)
    eng = _engine(st)
    try:
        got = eng.source_lh_by_feature(0)
    finally:
        eng.close()
    want, bound = cc.slf_double(st)
    fin = np.isfinite(want)
    assert got.dtype == F32 and np.array_equal(np.isneginf(got), ~fin) and not np.isnan(got).any(), (got, want)
    err = np.abs(got[fin].astype(np.float64) - want[fin])
    ratio = err / bound[fin]
    print(f"[clusterop] source_lh_by_feature N={N} F={F}: largest error / bound {ratio.max():.3f} (error {err[ratio.argmax()]:.3e}), "
          f"-inf at {np.flatnonzero(~fin).tolist()}")
    assert (err <= bound[fin]).all(), (got, want, bound)
    assert got[0] == -math.inf and got[F - 1] == -math.inf and got[1] == 0.0
