"""The cases of tests/_srcdraw_range_cases.py are what they claim to be -- proved with the oracle-backed double alone (no GPU):
the probability range is reached (exact zeros, denormals, no all-zero row), the planted uniforms sit ON the steps of the
double's float32 cdf and reach every component and every kind, a `<=` in place of the `<` would draw differently there, the
tempered uniforms are clear of the steps, the -inf and the failing states fail where and as often as stated, the shapes sit on
the edges they name.  tests/test_gpu_srcdraw_range.py then holds the device to the double on exactly these cases."""
import math

import numpy as np
import pytest

from oracle import sbayes_oracle as orc
from tests import _srcdraw_range_cases as sc


def _rows(C, from_prior=False, t=1.0, tp=1.0):
    st = sc.range_state(C)
    fake = sc.double_of(st)
    objs = np.arange(st.shape[0])
    return st, fake, objs, fake._source_probs(0, objs, t, tp, from_prior)


@pytest.mark.parametrize("C", [8, 5, 2])
def test_probability_range_is_reached(C):
    st, fake, objs, p = _rows(C)
    w = st.weights.astype(np.float64)
    assert (w == 0).any() and ((w > 0) & (w < sc.TINY)).any() and (w == sc.TINY).any()
    assert (w.max(axis=1) / np.where(w > 0, w, np.inf).min(axis=1) >= 1e59).any()          # the 1e30 / 1e-30 spread within one row
    assert st.na.any()
    hc = st.has_components
    assert not hc.all(axis=0)[[c for c in range(C) if c != sc.UNIVERSAL]].any()              # every other component: some object in no group
    tables = orc.component_probs(st.counts[0], st.conc[0])
    assert (tables[:, st.unif > 0] == 0).any() and ((tables > 0) & (tables < sc.TINY)).any()   # table entries 0 and denormal
    zero, denormal = sc.zero_and_denormal_share(p)
    assert zero >= 0.01 and denormal >= 0.01, (zero, denormal)
    assert np.isfinite(p).all() and (p.sum(axis=-1) > 0).all()                               # no row fails normalize
    cdf = sc.steps_of(p)
    assert (cdf[..., -1] == 1).all()
    # the cluster operators' rows on the same state: the same range
    hc_new, hc_old, src_old, gid_old, gid_new = sc.gu_inputs(st, objs, 1)
    assert (hc_new[:, 0] != hc_old[:, 0]).sum() == (objs.size + 1) // 2
    for k in range(2):
        q, q_back = fake.given_unchanged_probs(0, k, objs, hc_new, hc_old)
        for rows in (q, q_back):
            zero, denormal = sc.zero_and_denormal_share(rows)
            assert zero >= 0.01 and denormal >= 0.01 and (rows.sum(axis=-1) > 0).all(), (k, zero, denormal)
        # ... and the new method of the double is the rows given_unchanged_gibbs draws from
        z = np.random.default_rng(k).random(q.shape[:2])
        ids, sel, back = fake.given_unchanged_gibbs(0, k, objs, hc_new, hc_old, src_old, z)
        na = st.na
        assert np.array_equal(ids[~na], orc.sample_categorical(q, z)[~na])
        assert np.array_equal(sel[~na], np.take_along_axis(q, ids.astype(np.int64)[..., None] % C, axis=-1)[..., 0][~na])
        has_old = src_old != 255
        assert np.array_equal(back[has_old], np.take_along_axis(q_back, src_old.astype(np.int64)[..., None] % C, axis=-1)[..., 0][has_old])


def _check_planted(p, na, seed, kinds):
    C = p.shape[-1]
    cdf = sc.steps_of(p)
    z, kind, comp = sc.plant(p, seed)
    draw = orc.sample_categorical(p, z)
    valid = ~na
    for k in kinds:
        assert (kind[valid] == k).sum() >= 20, (sc.KINDS[k], int((kind[valid] == k).sum()))
    assert set(np.unique(draw[valid])) == set(range(C))                                      # every component is drawn somewhere
    sel = np.take_along_axis(p, draw[..., None], axis=-1)[..., 0]
    assert (sel[valid & (z < 1)] > 0).all()                                                  # never a zero-probability component
    at = np.take_along_axis(cdf, comp[..., None], axis=-1)[..., 0].astype(np.float64)
    reached = np.take_along_axis(cdf, draw[..., None], axis=-1)[..., 0].astype(np.float64)
    on = np.isin(kind, (sc.ON, sc.TIE)) & (z < 1)
    assert (z[on] == at[on]).all() and (draw[on] > comp[on]).all() and (reached[on] > at[on]).all()     # ON the step: the next one up
    tie = kind == sc.TIE
    assert (draw[tie] > comp[tie] + 1).all()                                                 # ... stepping over the tied component
    below = kind == sc.BELOW
    assert (z[below] < at[below]).all() and (reached[below] == at[below]).all() and (draw[below] <= comp[below]).all()
    assert (np.nextafter(z[below], 2.0) == at[below]).all()                                  # one double below the step
    assert (z[kind == sc.TIE_TOP] == 1.0).all() and (draw[kind == sc.TIE_TOP] == 0).all()
    top = kind == sc.TOPK
    assert (z[top] == sc.TOP).all() and (reached[top] == 1).all() and (sel[top] > 0).all()
    zero = kind == sc.ZERO
    assert (z[zero] == 0).all() and (draw[zero] == 0).all()
    cdf0 = kind == sc.CDF0
    assert (z[cdf0] == 0).all() and (cdf[cdf0][:, 0] == 0).all() and (draw[cdf0] > 0).all()
    # a comparison by `<=` draws another component on the steps: the kinds that catch it
    wrong = np.argmax(z[..., None] <= cdf, axis=-1)
    caught = on | cdf0 | ((kind == sc.TIE_TOP) & (cdf[..., 0] < 1))
    assert (caught & valid).sum() >= 40 and (wrong != draw)[caught].all()
    return z, kind


@pytest.mark.parametrize("C", [8, 5, 2])
def test_planted_uniforms_reach_every_step_kind(C):
    st, fake, objs, p = _rows(C)
    kinds = range(7) if C > 2 else (sc.ON, sc.BELOW, sc.ZERO, sc.TOPK, sc.CDF0)              # (C = 2: a tie would need p[universal] = 0)
    _check_planted(p, st.na, 1, kinds)
    hc_new, hc_old, *_ = sc.gu_inputs(st, objs, 1)
    q, _ = fake.given_unchanged_probs(0, 0, objs, hc_new, hc_old)
    _check_planted(q, st.na, 1, kinds)


@pytest.mark.parametrize("C", [8, 5, 2])
@pytest.mark.parametrize("temps", sc.TEMPERATURES, ids=lambda v: f"T{v[0]}-Tp{v[1]}")
def test_tempered_uniforms_are_clear_of_the_steps(C, temps):
    """Planted: every uniform at least 1e-4 from every step of the double's tempered cdf, so the GPU test excludes none; random:
    at most 1 % within 1e-5 of a step."""
    t, tp = temps
    st, fake, objs, p = _rows(C, t=t, tp=tp)
    z = sc.plant_clear(p, 3)
    d = sc.distance_to_steps(p, z)
    assert (z > 0).all() and (z < 1).all() and (d >= sc.CLEAR).all() and (d <= 1.11 * sc.CLEAR).mean() >= 0.5
    z = np.random.default_rng(4).random(p.shape[:2])
    assert (sc.distance_to_steps(p, z) <= sc.NEAR).mean() <= 0.01
    hc_new, hc_old, *_ = sc.gu_inputs(st, objs[:33], 6)
    q, _ = fake.given_unchanged_probs(0, 1, objs[:33], hc_new, hc_old, t, tp)
    assert (sc.distance_to_steps(q, sc.plant_clear(q, 6)) >= sc.CLEAR).all()


@pytest.mark.parametrize("C", [8, 5, 2])
@pytest.mark.parametrize("tp", [1.0, 1.7])
def test_from_prior_rows_have_zero_weights(C, tp):
    st, fake, objs, p = _rows(C, from_prior=True, tp=tp)
    assert ((p == 0) & st.has_components[:, None, :]).sum() >= 20
    assert (p.sum(axis=-1) > 0).all() and np.isfinite(p).all()
    if tp == 1.0:
        _check_planted(p, st.na, 7, (sc.ON, sc.BELOW, sc.ZERO, sc.TOPK, sc.CDF0))
    else:
        assert (sc.distance_to_steps(p, sc.plant_clear(p, 7)) >= sc.CLEAR).all()


def test_log_q_back_state_selects_zeros():
    st = sc.logq_state()
    fake = sc.double_of(st)
    N, F, C = st.shape
    objs = np.arange(N)
    log_q, sel = fake.source_logprob(0, 0, objs, return_selected=True)
    assert (sel == 0).sum() >= 20 and log_q == -math.inf and sc.fsum_log(sel, st.na) == -math.inf
    z = np.random.default_rng(12).random((N, F))
    ids, fwd, back, touched, rows = fake.gibbs_propose(0, 1, objs, z)
    assert (back == 0).sum() >= 20 and (fwd > 0).all() and math.isfinite(sc.fsum_log(fwd, st.na))
    hc_new, hc_old, src_old, _, _ = sc.gu_inputs(st, objs, 13)
    assert (fake.given_unchanged_gibbs(0, 0, objs, hc_new, hc_old, src_old, z)[2] == 0).sum() >= 20


@pytest.mark.parametrize("k", [1, 3])
def test_failing_state_fails_in_exactly_k_observations(k):
    bad, good, objs, spots = sc.fail_state(k)
    assert len(spots) == k and list(objs) == sorted(objs)
    N, F, C = bad.shape
    assert len({(r * F + f) // 256 for r, f in spots}) == k and len({f // 16 for _, f in spots}) == k   # different blocks, different tiles
    fake = sc.double_of(bad)
    with pytest.raises(AssertionError):
        fake.source_posterior(0, objs)
    with pytest.raises(AssertionError):
        fake.gibbs_propose(0, 1, objs, np.zeros((objs.size, F)))
    # the terms of the posterior, before normalize: exact zeros in exactly the k rows, nothing that is not a number
    groups, weights, lh = fake._state(0)
    w = orc.normalize_weights(weights, orc.has_components(groups))
    terms = lh[objs] * w[objs]
    assert np.isfinite(terms).all() and (terms >= 0).all()
    dead = np.argwhere(terms.sum(axis=-1) == 0)
    assert {(int(r), int(f)) for r, f in dead} == set(spots)
    assert (terms[dead[:, 0], dead[:, 1]] == 0).all()
    assert (lh[np.setdiff1d(np.arange(N), objs)] * w[np.setdiff1d(np.arange(N), objs)]).sum(axis=-1).min() > 0
    # the cluster operators' form, for every cluster: the same k rows, in both samples' weights
    hc = bad.has_components[objs]
    for i_cluster in range(bad.n_groups[0]):
        glh = fake.given_unchanged_lh(0, i_cluster, objs)
        gterms = glh * orc.normalize_weights(bad.weights, hc)
        assert np.isfinite(gterms).all()
        assert {(int(r), int(f)) for r, f in np.argwhere(gterms.sum(axis=-1) == 0)} == set(spots)
        with pytest.raises(AssertionError):
            fake.given_unchanged_probs(0, i_cluster, objs, hc, hc)
    # after the forward draw (component 0 where nothing exceeds z) the backward rows are positive: the proposal meets k rows, once
    cand = bad.source.copy()
    for r, f in spots:
        cand[objs[r], f] = np.eye(C, dtype=bool)[0]
    counts = orc.recalculate_feature_counts(bad.features, bad.groups, cand)
    lh2 = orc.likelihood_per_component(bad.features, bad.na, bad.groups, counts, bad.conc)
    assert (lh2[objs] * w[objs]).sum(axis=-1).min() > 0
    # the repaired state on the same feature block
    assert np.array_equal(good.features, bad.features)
    p = sc.double_of(good).source_posterior(0, objs)
    assert (p.sum(axis=-1) > 0).all()


@pytest.mark.parametrize("name", list(sc.EDGE_SHAPES))
def test_edge_shapes_sit_on_the_edges(name):
    st, sizes = sc.edge_state(name)
    N, F, C = st.shape
    assert F % 64 != 0 and N <= 70 or name == "f1"
    assert max(sizes) <= N
    p = sc.double_of(st).source_posterior(0, np.arange(N))
    assert (p.sum(axis=-1) > 0).all()
    for size in sizes:
        asc, shuffled = sc.subsets(N, size, 20 + size)
        assert list(asc) == sorted(set(asc)) and sorted(shuffled) == list(asc) and (size < 3 or list(shuffled) != list(asc))


def test_edges_are_all_there():
    shapes = {name: (shape, sizes) for name, (shape, sizes) in sc.EDGE_SHAPES.items()}
    products = {size * shape[1] for shape, sizes in shapes.values() for size in sizes}
    assert {1, 255, 256, 257} <= products                                                    # n_sub F around the 256-thread block
    assert {shape[1] for shape, _ in shapes.values()} == {1, 15, 16, 17, 33}                 # F around the 16-feature tile
    assert all({1, 64, 65} <= set(sizes) for (shape, sizes) in shapes.values() if shape[1] > 1)   # n_sub 16 around the 1024-thread block
    assert {shape[2] for shape, _ in shapes.values()} >= {8, 9, 16, 17}                      # S: the three table-rebuild paths
    st = sc.single_component_state()
    assert st.shape[2] == 1 and st.has_components.all()
    p = sc.double_of(st).source_posterior(0, np.arange(st.shape[0]))
    assert (p == 1).all() and (sc.steps_of(p) == 1).all()
