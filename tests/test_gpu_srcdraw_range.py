"""The Gibbs source draw over its probability, uniform and shape range: the three hand-written forms of "posterior row over the
components, float32 cdf, first component whose cdf exceeds the uniform" (sbayes_amd/csrc/sbe_kernels_sampling.hip.h) against
the oracle-backed double (tests/_fake_engine.py), on the cases of tests/_srcdraw_range_cases.py -- tests/test_srcdraw_range_cpu.py
proves with the double alone that the cases are what they claim to be.  DESIGN.md section 4.3a.

    chain form   k_source_posterior / k_sample_source / k_source_logprob   source_posterior, sample_source, source_logprob,
                                                                           gibbs_propose(fuse_tables=False), gibbs_step
    tile form    k_gibbs_propose_tile                                      gibbs_propose(fuse_tables=True)
    cluster form k_given_unchanged_gibbs / k_given_unchanged_fused         given_unchanged_gibbs(fuse_tables=False / True)

At T = T_prior = 1 ids, selected probabilities, touched groups and count rows are the double's bit for bit, with uniforms ON the
steps of the double's float32 cdf.  Tempered, probabilities agree to 2e-6 relative (float32 powf; floor 2^-147) and every draw
is the double's where the uniform is farther than 1e-5 from every step -- the planted ones all are.  log_q is within 1e-12
relative of the exactly rounded sum of the float64 logs of the float32 selected probabilities.

Which test fails under which change of the kernels (reasoned from the code, not run):
    `zz < cdf / last` -> `<=`     test_planted_uniforms, test_from_prior[*-1.0], test_single_component: a uniform ON a step (kinds
                                  on, tie, tie_top, cdf0) then draws the component AT the step.  In k_sample_source: "sample_source
                                  ids", "gibbs_propose chain ids", "gibbs_step ids"; in k_gibbs_propose_tile: "gibbs_propose tile
                                  ids" and "tile form != chain form"; in gu_gibbs_obs (both cluster kernels run it): "given_unchanged
                                  ids".  tests/test_srcdraw_range_cpu.py shows that `<=` draws another component at every such uniform.
    no `c < C` in a cdf loop      The SUM loop: k_sample_source and k_gibbs_propose_tile leave p[C..7] unwritten (posterior_row_core
                                  stores c < C only), so without the guard `last` takes whatever those registers hold -- the cases
                                  with C < 8 run it: test_planted_uniforms[5], [2], test_from_prior, test_shape_edges and
                                  test_normalize_fails (C = 3), test_single_component (C = 1), ids and p_selected bit for bit.  In
                                  gu_gibbs_obs p[.][c >= C] is computed and is 0 / tot = +0, so the guard changes no result there;
                                  the guard of the COMPARISON loop changes none in any form either: behind C - 1 the cdf equals
                                  `last`, and z < 1 holds at C - 1 whenever it holds there.
    `sel` starts at 0 for NA      every test (every state has NA observations; asserted: p_selected is 1 and the id 255 there, in
                                  every form) -- "NA observations", and log_q turns -inf against a finite sum.
"""
import math

import numpy as np
import pytest

from oracle import sbayes_oracle as orc
from sbayes_amd.engine import Engine, EngineError
from tests import _srcdraw_range_cases as sc

pytestmark = pytest.mark.gpu

RTOL, FLOOR = 2e-6, 2.0 ** -147          # float32 powf as the existing tests bound it; two denormal steps
SBE_ERR_DATA = 4


def _pair(st):
    eng = sc.load(Engine(st.features, st.n_groups, n_slots=3), st)
    return eng, sc.double_of(st)


def _same(got, want, exact, what, where=None):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.dtype, want.dtype, got.shape, want.shape)
    if where is not None:
        got, want = got[where], want[where]
    if exact:
        assert np.array_equal(got, want), (what, int((got != want).sum()), "of", got.size)
    else:
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=FLOOR, err_msg=str(what))


def _close_logq(got, want, rel, what):
    if math.isinf(want) or math.isnan(want):
        assert got == want, (what, got, want)
    else:
        assert abs(got - want) <= rel * abs(want), (what, got, want)


def _check_source_forms(eng, fake, st, objs, z, t=1.0, tp=1.0, from_prior=False, far=None):
    """Every call of the chain and the tile form for one subset and one block of uniforms.  `far`: where the double's draw binds
    a tempered device (None: everywhere)."""
    exact = t == 1.0 and tp == 1.0
    tag = (st.name, len(objs), t, tp, from_prior)
    N, F, C = st.shape
    everyone = np.arange(N, dtype=np.int32)
    na = st.na[objs]
    if far is None:
        far = np.ones(na.shape, dtype=bool)
    assert far.all() or not exact
    # source_posterior
    if not from_prior:
        _same(eng.source_posterior(0, objs, t, tp), fake.source_posterior(0, objs, t, tp), exact, tag + ("source_posterior",))
    # sample_source: ids through the destination slot's rows, p[drawn], log_q
    for e in (eng, fake):
        e.copy_slot(1, 0)
    log_q, sel = eng.sample_source(0, 1, objs, z, t, tp, from_prior, return_selected=True)
    _, want_sel = fake.sample_source(0, 1, objs, z, t, tp, from_prior, return_selected=True)
    ids = sc.ids_of(eng.get_source_rows(1, objs))
    want_ids = sc.ids_of(fake.get_source_rows(1, objs))
    _same(ids, want_ids, True, tag + ("sample_source ids",), far)
    assert (ids[na] == 255).all() and (sel[na] == 1.0).all(), tag + ("NA observations",)
    _same(sel, want_sel, exact, tag + ("sample_source p_selected",), far)
    _close_logq(log_q, sc.fsum_log(want_sel if exact else sel, na), 1e-12, tag + ("sample_source log_q",))
    others = np.setdiff1d(everyone, objs)
    assert np.array_equal(eng.get_source_rows(1, others), st.source[others]), tag + ("rows outside the subset",)
    if not far.all():
        return                                        # (a draw that may differ leaves another candidate: nothing below is comparable)
    # source_logprob: the candidate's posterior at the current source
    eng.update_counts(1, 0, objs)
    fake.update_counts(1, 0, objs)
    for c in range(C):
        eng.update_probs(1, c)
    log_q_back, back = eng.source_logprob(1, 0, objs, t, tp, from_prior, return_selected=True)
    _, want_back = fake.source_logprob(1, 0, objs, t, tp, from_prior, return_selected=True)
    _same(back, want_back, exact, tag + ("source_logprob p_selected",))
    _close_logq(log_q_back, sc.fsum_log(want_back if exact else back, na), 1e-12, tag + ("source_logprob log_q",))
    # gibbs_propose: one kernel per feature tile / the chain that builds the candidate slot
    want = fake.gibbs_propose(0, 1, objs, z, t, tp, from_prior)
    names = ("ids", "sel", "sel_back", "touched", "rows")
    results = []
    for tile_form in (True, False):
        eng.set_option(fuse_tables=tile_form)
        got = eng.gibbs_propose(0, 1, objs, z, t, tp, from_prior)
        results.append(got)
        form = "tile" if tile_form else "chain"
        for name, g, w in zip(names, got, want):
            _same(g, w, exact or name in ("ids", "touched", "rows"), tag + (f"gibbs_propose {form} {name}",))
        assert np.array_equal(eng.get_source_rows(0, everyone), st.source), tag + (form, "the current slot changed")
    for name, a, b in zip(names, *results):
        assert np.array_equal(a, b), tag + ("tile form != chain form", name)
    assert np.array_equal(results[1][1], sel) and np.array_equal(results[1][2], back), tag + ("gibbs_propose != the two calls",)
    # ... with the current slot following: the same arrays, and the slot ends as the candidate
    for tile_form in (True, False):
        eng.set_option(fuse_tables=tile_form)
        eng.copy_slot(2, 0)
        got = eng.gibbs_propose(2, 1, objs, z, t, tp, from_prior, follow=True)
        for name, a, b in zip(names, got, results[0]):
            assert np.array_equal(a, b), tag + ("follow", tile_form, name)
        if got[3].size:
            assert np.array_equal(eng.get_source_rows(2, everyone), fake.get_source_rows(1, everyone)), tag + ("follow: source rows", tile_form)
            for c in range(C):
                assert np.array_equal(eng.get_counts(2, c), fake._slot(1)["counts"][c]), tag + ("follow: counts", c, tile_form)
            assert np.array_equal(eng.likelihood_per_component(2), fake._state(1)[2]), tag + ("follow: tables", tile_form)
    eng.set_option(fuse_tables=True)
    # gibbs_step: the sums of the same logs, by another tree
    log_q3, log_q_back3 = eng.gibbs_step(0, 1, objs, z, t, tp, from_prior)[:2]
    _close_logq(log_q3, log_q, 1e-13, tag + ("gibbs_step log_q",))
    _close_logq(log_q_back3, log_q_back, 1e-13, tag + ("gibbs_step log_q_back",))
    assert np.array_equal(sc.ids_of(eng.get_source_rows(1, objs)), want_ids), tag + ("gibbs_step ids",)


def _check_cluster_form(eng, fake, st, objs, i_cluster, seed, t=1.0, tp=1.0, from_prior=False, planted=True):
    """given_unchanged_gibbs plain and with its count delta, fused and not, hc_old differing from hc_new on half the subset; the
    uniforms are planted on the steps of THIS form's own rows (tempered: clear of them)."""
    exact = t == 1.0 and tp == 1.0
    tag = (st.name, len(objs), i_cluster, t, tp, from_prior)
    hc_new, hc_old, src_old, gid_old, gid_new = sc.gu_inputs(st, objs, seed)
    p, _ = fake.given_unchanged_probs(0, i_cluster, objs, hc_new, hc_old, t, tp, from_prior)
    if not planted:
        z = np.random.default_rng(seed).random(p.shape[:2])
    else:
        z = sc.plant(p, seed)[0] if exact else sc.plant_clear(p, seed)
    assert exact or (sc.distance_to_steps(p, z) > sc.NEAR).all()
    want = fake.given_unchanged_gibbs(0, i_cluster, objs, hc_new, hc_old, src_old, z, t, tp, from_prior, gid_old=gid_old, gid_new=gid_new)
    names = ("ids", "sel", "back", "touched", "rows")
    results = []
    for fuse in (True, False):
        eng.set_option(fuse_tables=fuse)
        plain = eng.given_unchanged_gibbs(0, i_cluster, objs, hc_new, hc_old, src_old, z, t, tp, from_prior)
        full = eng.given_unchanged_gibbs(0, i_cluster, objs, hc_new, hc_old, src_old, z, t, tp, from_prior, gid_old=gid_old, gid_new=gid_new)
        results.append(full)
        for name, a, b in zip(names, plain, full):
            assert np.array_equal(a, b), tag + (fuse, "draw differs with the count delta asked for", name)
        for name, g, w in zip(names, full, want):
            _same(g, w, exact or name in ("ids", "touched", "rows"), tag + (f"given_unchanged {name}", "fused" if fuse else "two launches"))
        na = st.na[objs]
        assert (full[0][na] == 255).all() and (full[1][na] == 1.0).all(), tag + ("NA observations",)
    eng.set_option(fuse_tables=True)
    for name, a, b in zip(names, *results):
        assert np.array_equal(a, b), tag + ("fused != two launches", name)


# ---- 1 + 2: the probability range, uniforms on the steps, T = T_prior = 1 ------------------------------------------------------
@pytest.mark.parametrize("C", [8, 5, 2])
def test_planted_uniforms(C):
    """Weights of exactly 0, denormal, 2^-126 and a 1e30 / 1e-30 spread, table entries of 0 and denormal, objects without a group,
    NA observations -- and every uniform ON a step of the double's float32 cdf, one double below it, 0, 1 - 2^-53, on tied steps
    or on a first step of 0: the three forms draw what the double draws and select its float32 probabilities, bit for bit."""
    st = sc.range_state(C)
    eng, fake = _pair(st)
    try:
        N = st.shape[0]
        for size, seed in ((N, 1), (17, 2)):
            asc, shuffled = sc.subsets(N, size, seed)
            objs = asc if size == N else shuffled                 # (the smaller subset is given unsorted)
            z, _, _ = sc.plant(fake.source_posterior(0, objs), seed)
            _check_source_forms(eng, fake, st, objs, z)
            # ... and with the uniforms ON the top step (1.0: they select a probability of 0 where p[0] is 0, log_q = -inf) moved
            # to 1 - 2^-53: every selected probability positive, down to denormals, and log_q finite
            inside = np.where(z == 1.0, sc.TOP, z)
            log_q = fake.sample_source(0, 1, objs, inside)
            assert math.isfinite(log_q) and log_q < 0
            _check_source_forms(eng, fake, st, objs, inside)
            for i_cluster in range(2):
                _check_cluster_form(eng, fake, st, asc, i_cluster, seed + 10 * i_cluster)
    finally:
        eng.close()


def test_device_stream_on_the_range_state():
    """z = None: the engine's Philox stream on the probability-range state draws sample_categorical(p, philox_uniforms)."""
    st = sc.range_state(8)
    eng, fake = _pair(st)
    try:
        N, F, _ = st.shape
        objs = np.arange(N, dtype=np.int32)
        eng.set_rng(seed=0x0DDB1A5E5BAD5EED, draw=7)
        u = orc.philox_uniforms(0x0DDB1A5E5BAD5EED, 7, N * F).reshape(N, F)
        for e, z in ((eng, None), (fake, u)):
            e.copy_slot(1, 0)
        log_q, sel = eng.sample_source(0, 1, objs, None, return_selected=True)
        _, want_sel = fake.sample_source(0, 1, objs, u, return_selected=True)
        assert np.array_equal(sc.ids_of(eng.get_source_rows(1, objs)), sc.ids_of(fake.get_source_rows(1, objs)))
        assert np.array_equal(sel, want_sel)
        _close_logq(log_q, sc.fsum_log(want_sel, st.na), 1e-12, "log_q")
        assert eng.get_rng() == (0x0DDB1A5E5BAD5EED, 8)
    finally:
        eng.close()


# ---- 3: tempered -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [8, 5, 2])
@pytest.mark.parametrize("temps", sc.TEMPERATURES, ids=lambda v: f"T{v[0]}-Tp{v[1]}")
def test_tempered(C, temps):
    """The same states at (T, T_prior): probabilities to 2e-6 relative with a floor of 2^-147 (measured on the MI355X at these
    weights: 2.4e-7 in the chain and tile forms, 3.4e-7 in the cluster form, denormal entries bit-equal -- DESIGN.md 4.3a), and with uniforms 1e-4 from the steps every draw is the double's in every form.
    Random uniforms: the double's draw wherever the uniform is farther than 1e-5 from each of its steps."""
    t, tp = temps
    st = sc.range_state(C)
    eng, fake = _pair(st)
    try:
        N = st.shape[0]
        objs = np.arange(N, dtype=np.int32)
        p = fake.source_posterior(0, objs, t, tp)
        _check_source_forms(eng, fake, st, objs, sc.plant_clear(p, 3), t, tp)
        z = np.random.default_rng(4).random(p.shape[:2])
        _check_source_forms(eng, fake, st, objs, z, t, tp, far=sc.distance_to_steps(p, z) > sc.NEAR)
        asc, _ = sc.subsets(N, 33, 5)
        _check_cluster_form(eng, fake, st, asc, 1, 6, t, tp)
    finally:
        eng.close()


# ---- 4: from_prior -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [8, 5, 2])
@pytest.mark.parametrize("tp", [1.0, 1.7])
def test_from_prior(C, tp):
    """sample_from_prior: the all-float32 path, the weights alone (rows with a zero weight in a component the object has)."""
    st = sc.range_state(C)
    eng, fake = _pair(st)
    try:
        N = st.shape[0]
        objs = np.arange(N, dtype=np.int32)
        p = fake._source_probs(0, objs, 1.0, tp, True)
        assert ((p == 0) & st.has_components[:, None, :]).any()
        z = sc.plant(p, 7)[0] if tp == 1.0 else sc.plant_clear(p, 7)
        _check_source_forms(eng, fake, st, objs, z, 1.0, tp, from_prior=True)
        asc, _ = sc.subsets(N, 33, 8)
        _check_cluster_form(eng, fake, st, asc, 0, 9, 1.0, tp, from_prior=True)
    finally:
        eng.close()


# ---- 5: log_q_back = -inf ------------------------------------------------------------------------------------------------------------
def test_log_q_back_minus_infinity():
    """The current source points at components of probability exactly 0: the backward probability selected there is 0.0, its log
    -inf, the sum -inf -- not NaN, not an error -- and every other selected probability is still the double's."""
    st = sc.logq_state()
    eng, fake = _pair(st)
    try:
        N, F, C = st.shape
        objs = np.arange(N, dtype=np.int32)
        z = np.random.default_rng(12).random((N, F))
        # source_logprob of the state at its own source
        log_q, sel = eng.source_logprob(0, 0, objs, return_selected=True)
        _, want = fake.source_logprob(0, 0, objs, return_selected=True)
        assert (want == 0).sum() >= 20
        assert np.array_equal(sel, want) and log_q == -math.inf
        # the backward pass of the proposal, both forms, and the one-call step
        want = fake.gibbs_propose(0, 1, objs, z)
        assert (want[2] == 0).sum() >= 20
        for tile_form in (True, False):
            eng.set_option(fuse_tables=tile_form)
            got = eng.gibbs_propose(0, 1, objs, z)
            for g, w in zip(got, want):
                assert np.array_equal(g, w), tile_form
        eng.set_option(fuse_tables=True)
        log_q, log_q_back = eng.gibbs_step(0, 1, objs, z)[:2]
        assert log_q_back == -math.inf
        _close_logq(log_q, sc.fsum_log(want[1], st.na), 1e-12, "gibbs_step log_q")
        hc_new, hc_old, src_old, _, _ = sc.gu_inputs(st, objs, 13)
        want = fake.given_unchanged_gibbs(0, 0, objs, hc_new, hc_old, src_old, z)
        assert (want[2] == 0).sum() >= 20
        for fuse in (True, False):
            eng.set_option(fuse_tables=fuse)
            for g, w in zip(eng.given_unchanged_gibbs(0, 0, objs, hc_new, hc_old, src_old, z), want):
                assert np.array_equal(g, w), fuse
    finally:
        eng.close()


# ---- 6: normalize fails --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3])
def test_normalize_fails(k):
    """Exactly k observations (different blocks of 256, different feature tiles) whose every component has likelihood x weight 0:
    the double raises normalize's AssertionError; the device fails in the CALL that met them (every form waits for its own
    kernels and reads the status words then: sbe_engine_internal.hip.h, read_status / take_status / sync_and_report) with
    SBE_ERR_DATA and the count k -- the proposal too: the rows that failed forward draw component 0 (nothing exceeds z in a NaN
    cdf), whose count then makes the backward row positive.  The status does not stick: the same call on the other objects, and
    every call on the repaired state, answer like the double."""
    bad, good, objs, spots = sc.fail_state(k)
    eng, fake = _pair(bad)
    try:
        N, F, C = bad.shape
        z = np.random.default_rng(14).random((objs.size, F))
        hc_new, hc_old, src_old, gid_old, gid_new = sc.gu_inputs(bad, objs, 15)
        hc_old, gid_old = hc_new, gid_new                           # (both samples alike: a failing row is one row)
        clean = np.array([o for r, o in enumerate(objs) if r not in {r for r, _ in spots}], dtype=np.int32)
        message = rf"normalize: {k} (observations|rows) have a non-positive"

        def fails(call):
            with pytest.raises(EngineError, match=message) as err:
                call()
            assert err.value.code == SBE_ERR_DATA
            # the next call starts from cleared status words
            assert np.array_equal(eng.source_posterior(0, clean), fake.source_posterior(0, clean))

        with pytest.raises(AssertionError):
            fake.source_posterior(0, objs)
        with pytest.raises(AssertionError):
            fake.given_unchanged_gibbs(0, 0, objs, hc_new, hc_old, src_old, z)
        eng.copy_slot(1, 0)
        fails(lambda: eng.source_posterior(0, objs))
        fails(lambda: eng.sample_source(0, 1, objs, z))
        fails(lambda: eng.source_logprob(0, 0, objs))
        for tile_form in (True, False):
            eng.set_option(fuse_tables=tile_form)
            fails(lambda: eng.gibbs_propose(0, 1, objs, z))
        for fuse in (True, False):
            eng.set_option(fuse_tables=fuse)
            fails(lambda: eng.given_unchanged_gibbs(0, 0, objs, hc_new, hc_old, src_old, z))
            fails(lambda: eng.given_unchanged_gibbs(0, 0, objs, hc_new, hc_old, src_old, z, gid_old=gid_old, gid_new=gid_new))
        eng.set_option(fuse_tables=True)
        # SBE_OPT_DEFERRED_CHECKS defers the reports of state-setting calls; these calls wait for their own results and report
        # their own rows, in the same words, and leave nothing pending
        eng.set_option(deferred_checks=True)
        fails(lambda: eng.source_posterior(0, objs))
        fails(lambda: eng.gibbs_propose(0, 1, objs, z))
        fails(lambda: eng.given_unchanged_gibbs(0, 0, objs, hc_new, hc_old, src_old, z))
        eng.set_option(fuse_tables=False)
        fails(lambda: eng.gibbs_propose(0, 1, objs, z))
        eng.set_option(fuse_tables=True, deferred_checks=False)
        # the same handle on the repaired state
        sc.load(eng, good)
        fake = sc.double_of(good)
        _check_source_forms(eng, fake, good, objs, z)
        _check_cluster_form(eng, fake, good, objs, 0, 16, planted=False)
    finally:
        eng.close()


# ---- 7: shape edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.EDGE_SHAPES))
def test_shape_edges(name):
    """Ordinary states at n_sub F = 1, 255, 256, 257 (the 256-thread blocks and their inactive lanes), F = 1, 15, 16, 17, 33 (the
    16-feature tile), n_sub = 1, 64, 65 (the 1024-thread tile block and its prefetched first uniform), S = 8, 9, 16, 17 (the three
    table-rebuild paths), subsets given unsorted; F is never a multiple of 64, so the padded row pitch differs from F."""
    st, sizes = sc.edge_state(name)
    eng, fake = _pair(st)
    try:
        N, F, _ = st.shape
        for size in sizes:
            asc, shuffled = sc.subsets(N, size, 20 + size)
            z = np.random.default_rng(30 + size).random((size, F))
            _check_source_forms(eng, fake, st, shuffled, z)
            _check_cluster_form(eng, fake, st, asc, size % 2, 40 + size, planted=size > 64)
    finally:
        eng.close()


def test_single_component():
    """C = 1: the cdf of every row is [1]; component 0 or NA, p_selected 1, log_q 0 -- at z = 0, on the step (1.0) and below it."""
    st = sc.single_component_state()
    eng, fake = _pair(st)
    try:
        N, F, _ = st.shape
        objs = np.arange(N, dtype=np.int32)
        z = sc.plant(fake.source_posterior(0, objs), 50)[0]
        assert (z == 1.0).any() and (z == 0.0).any()
        _check_source_forms(eng, fake, st, objs, z)
        _check_cluster_form(eng, fake, st, objs, 2, 51)
        log_q, sel = eng.sample_source(0, 1, objs, z, return_selected=True)
        assert log_q == 0.0 and (sel == 1.0).all()
        assert set(np.unique(sc.ids_of(eng.get_source_rows(1, objs)))) == {0, 255}
    finally:
        eng.close()
