"""The Gibbs weights step on the device (sbayes_amd.wgibbs, include/sbe_wgibbs.h) against tests/_wgibbs_oracle.py on the
reference's recorded proposals (tests/golden/wgibbs.npz) and on seeded synthetic states: counts and proposed weights
bit-exact, the log ratio inside the any-order float64 band, every decision and output row identical, results
bit-identical run to run, on any slot, for feature counts off the tile and object counts below and above one sweep."""
import ctypes as ct

import numpy as np
import pytest

from sbayes_amd import wgibbs
from sbayes_amd.engine import Engine, EngineError
from tests import _wgibbs_cases as wc
from tests import _wgibbs_oracle as worc

pytestmark = pytest.mark.gpu
SWEEP = 64 * 8                                            # objects one pass of a workgroup's 64 lanes covers


def make_engine(na, n_components, n_slots=1):
    """An engine whose resident block has exactly the NA mask `na`: one state, set where the observation is not missing
    (the step reads nothing else of the features); one group per component, so a component's group is has_components."""
    feats = np.zeros(na.shape + (2,), dtype=bool)
    feats[..., 0] = ~na
    return Engine(feats, [1] * n_components, n_slots=n_slots, device=0)


def bind(eng, slot, has_components, src, w):
    c = has_components.shape[1]
    for comp in range(c):
        eng.set_groups(slot, comp, has_components[:, comp][None, :])
    eng.set_source(slot, wc.source_array(src, c))
    eng.set_weights(slot, w)


def check_proposal(eng, slot, label, w, has_components, src, na, i1, i2, a2, u, alpha, beta_ab, t):
    """One proposal on the device against the restatement; returns what the device gave."""
    patterns, pid = np.unique(has_components, axis=0, return_inverse=True)
    pid = np.asarray(pid).reshape(-1)
    counts = wgibbs.pair_counts(eng, slot, i1, i2)
    want_counts = worc.pair_counts(patterns, pid, src, na, i1, i2)
    assert counts.dtype == np.int32 and np.array_equal(counts, want_counts), label
    want_out, want_accept, terms, want_new = worc.step(w, patterns, pid, src, na, i1, i2, a2, u, alpha, beta_ab, t)
    w_out, accept, log_p = wgibbs.step(eng, slot, i1, i2, a2, u, alpha, beta_ab, t)
    w_all, accept_all, _ = wgibbs.step(eng, slot, i1, i2, a2, np.zeros_like(u), alpha, beta_ab, t)   # u = 0: every p > 0 accepts
    band = worc.device_band(terms, t)
    margin = worc.log_margin(u, terms["log_p"])
    finite = np.isfinite(terms["log_p"])
    err = np.abs(log_p - terms["log_p"])[finite]
    print(f"[wgibbs] {label}: max |log_p dev - oracle| {err.max(initial=0.0):.3e}, largest err / band "
          f"{np.max(err / np.maximum(band[finite], 1e-300), initial=0.0):.3e}, least margin / band "
          f"{np.min(margin[finite] / np.maximum(band[finite], 1e-300), initial=np.inf):.3e}, accepted {int(accept.sum())} / {accept.size}")
    # no decision lies inside the band: nothing is excluded below.  (A feature whose log_p is NaN or infinite has no band --
    # S is NaN or infinite with it -- and no margin to speak of: its decision does not depend on u's distance from p, and
    # the device's log_p must be the same NaN or infinity, asserted below.)
    assert (margin[finite] > band[finite]).all(), label
    shown = accept_all & (np.exp(terms["log_p"]) > 0)
    assert shown.sum() >= accept.sum() and w_all[shown].tobytes() == want_new[shown].tobytes(), label   # w_new, bit for bit
    assert np.array_equal(np.isnan(log_p), np.isnan(terms["log_p"])), label
    assert np.array_equal(log_p[~finite & ~np.isnan(log_p)], terms["log_p"][~finite & ~np.isnan(log_p)]), label
    assert (err <= band[finite]).all(), (label, err.max())
    assert np.array_equal(accept, want_accept), label
    assert w_out.dtype == np.float32 and w_out.tobytes() == want_out.tobytes(), label
    return counts, w_out, accept, log_p


@pytest.mark.parametrize("tag", wc.CASES)
def test_device_against_oracle_on_the_recorded_proposals(tag):
    case = wc.load(tag)
    n, f, c = case["shape"]
    with make_engine(case["na"], c) as eng:
        for k, p in enumerate(case["proposals"]):
            bind(eng, 0, p["has_components"], p["src"], p["w"])
            counts, w_out, accept, _ = check_proposal(eng, 0, f"{tag}[{k}]", p["w"], p["has_components"], p["src"], case["na"],
                                                      p["i1"], p["i2"], p["a2"], p["u"], case["alpha"], p["beta_ab"],
                                                      case["prior_temperature"])
            # ... and against what the reference itself computed
            assert np.array_equal(counts, p["counts"]) and np.array_equal(accept, p["accept"])
            assert w_out.tobytes() == p["w_out"].tobytes()
            assert np.array_equal(eng.get_weights(0), p["w"])          # the slot is left untouched


def synthetic_state(seed, n, f, c, n_patterns=None, na_rate=0.15):
    rng = np.random.default_rng(seed)
    if n_patterns is None:
        hc = rng.random((n, c)) < 0.7
        hc[:, min(1, c - 1)] = True
    else:
        pool = np.unique(np.concatenate([np.ones((1, c), dtype=bool), rng.random((4 * n_patterns, c)) < 0.6]), axis=0)
        pool = pool[pool.any(axis=1)][:n_patterns]
        hc = pool[rng.integers(0, len(pool), n)]
    scores = rng.random((n, f, c)) * hc[:, None, :]
    src = scores.argmax(axis=-1).astype(np.int16)
    na = rng.random((n, f)) < na_rate
    src[na] = -1
    w = rng.dirichlet(np.ones(c) * 2, f).astype(np.float32)
    i1, i2 = (int(v) for v in rng.choice(c, 2, replace=False))
    alpha = rng.choice([0.3, 0.5, 1.0, 2.5], (f, c))
    patterns, pid = np.unique(hc, axis=0, return_inverse=True)
    counts = worc.pair_counts(patterns, np.asarray(pid).reshape(-1), src, na, i1, i2)
    t = float(rng.choice([1.0, 1.5]))
    beta_ab = worc.beta_parameters(counts, np.full((f, c), 0.5, dtype=np.float32), i1, i2, t)
    a2 = rng.beta(beta_ab[:, 0], beta_ab[:, 1])
    u = rng.random(f, dtype=np.float32)
    return dict(w=w, has_components=hc, src=src, na=na, i1=i1, i2=i2, a2=a2, u=u, alpha=alpha, beta_ab=beta_ab, t=t)


SHAPES = [  # seed, N, F, C, patterns: F off the 16-feature tile; N below one sweep, just above it and several sweeps
    (1, 37, 21, 3, None), (2, SWEEP - 1, 16, 2, None), (3, SWEEP + 1, 17, 4, None), (4, 3 * SWEEP + 5, 50, 4, None),
    (5, 1300, 33, 8, 40), (6, 900, 5, 8, 64), (7, 1, 1, 2, None)]


@pytest.mark.parametrize("seed,n,f,c,n_patterns", SHAPES)
def test_shapes_off_the_tile_and_around_one_sweep(seed, n, f, c, n_patterns):
    s = synthetic_state(seed, n, f, c, n_patterns)
    if n_patterns == 64:
        assert len(np.unique(s["has_components"], axis=0)) == 64      # the engine's pattern limit: the largest table in LDS
    with make_engine(s["na"], c) as eng:
        bind(eng, 0, s["has_components"], s["src"], s["w"])
        check_proposal(eng, 0, f"synthetic N={n} F={f} C={c}", s["w"], s["has_components"], s["src"], s["na"], s["i1"], s["i2"],
                       s["a2"], s["u"], s["alpha"], s["beta_ab"], s["t"])


def test_results_are_bit_identical_run_to_run_and_on_another_slot():
    case = wc.load("south_america")
    p, q = case["proposals"][0], case["proposals"][-1]
    n, f, c = case["shape"]
    args = (p["i1"], p["i2"], p["a2"], p["u"], case["alpha"], p["beta_ab"], case["prior_temperature"])
    with make_engine(case["na"], c, n_slots=3) as eng:
        bind(eng, 0, q["has_components"], q["src"], q["w"])           # another state in slot 0
        bind(eng, 2, p["has_components"], p["src"], p["w"])
        first = [wgibbs.pair_counts(eng, 2, p["i1"], p["i2"])] + list(wgibbs.step(eng, 2, *args))
        for _ in range(5):
            again = [wgibbs.pair_counts(eng, 2, p["i1"], p["i2"])] + list(wgibbs.step(eng, 2, *args))
            assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
        check_proposal(eng, 2, "slot 2", p["w"], p["has_components"], p["src"], case["na"], *args)
        other = wgibbs.step(eng, 0, q["i1"], q["i2"], q["a2"], q["u"], case["alpha"], q["beta_ab"], case["prior_temperature"])
        assert other[0].tobytes() == q["w_out"].tobytes()             # slot 0 still holds its own state
    with make_engine(case["na"], c) as eng:                           # a fresh engine, slot 0: the same bits
        bind(eng, 0, p["has_components"], p["src"], p["w"])
        fresh = [wgibbs.pair_counts(eng, 0, p["i1"], p["i2"])] + list(wgibbs.step(eng, 0, *args))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, fresh))
        w_out, accept, log_p = wgibbs.step(eng, 0, *args, want_log_p=False)
        assert log_p is None and w_out.tobytes() == first[1].tobytes() and np.array_equal(accept, first[2])


def test_a_state_with_an_empty_has_both_set():
    s = synthetic_state(11, 200, 20, 3)
    s["has_components"][:, 0] = np.arange(200) % 2 == 0              # no object has components 0 and 2 together
    s["has_components"][:, 2] = ~s["has_components"][:, 0]
    s["has_components"][:, 1] = True
    rng = np.random.default_rng(12)
    scores = rng.random((200, 20, 3)) * s["has_components"][:, None, :]
    s["src"] = scores.argmax(axis=-1).astype(np.int16)
    s["src"][s["na"]] = -1
    s["i1"], s["i2"] = 0, 2
    s["beta_ab"] = np.full((20, 2), 1.5)
    with make_engine(s["na"], 3) as eng:
        bind(eng, 0, s["has_components"], s["src"], s["w"])
        counts, *_ = check_proposal(eng, 0, "empty has_both", s["w"], s["has_components"], s["src"], s["na"], 0, 2, s["a2"], s["u"],
                                    s["alpha"], s["beta_ab"], s["t"])
        assert not counts.any()


def test_an_observation_without_a_source_component_rejects_its_feature():
    s = synthetic_state(13, 120, 18, 3)
    s["src"][5, 7] = -1
    s["na"][5, 7] = False
    with make_engine(s["na"], 3) as eng:
        bind(eng, 0, s["has_components"], s["src"], s["w"])
        _, w_out, accept, log_p = check_proposal(eng, 0, "no source", s["w"], s["has_components"], s["src"], s["na"], s["i1"], s["i2"],
                                                 s["a2"], np.zeros(18, dtype=np.float32), s["alpha"], s["beta_ab"], s["t"])
        assert np.isnan(log_p[7]) and not accept[7] and np.array_equal(w_out[7], s["w"][7])
        assert accept[np.arange(18) != 7].all()


def test_error_codes():
    s = synthetic_state(14, 40, 10, 3)
    lib = wgibbs.load()
    f, c = 10, 3
    a2, u, alpha, ab = s["a2"], s["u"], np.ascontiguousarray(s["alpha"]), np.ascontiguousarray(s["beta_ab"])
    w_out, acc, cnt = np.zeros((f, c), dtype=np.float32), np.zeros(f, dtype=np.uint8), np.zeros((f, 2), dtype=np.int32)
    ptr = lambda a: a.ctypes.data                          # noqa: E731

    def raw_step(eng, slot, i1, i2, t, a2_ptr=None):
        return lib.sbe_wgibbs_step(eng._h, slot, i1, i2, ptr(a2) if a2_ptr is None else a2_ptr, ptr(u), ptr(alpha), ptr(ab), t,
                                   ptr(w_out), ptr(acc), None)

    with make_engine(s["na"], c, n_slots=2) as eng:
        with pytest.raises(EngineError) as exc:            # SBE_ERR_STATE: nothing is set
            wgibbs.pair_counts(eng, 0, 0, 1)
        assert exc.value.code == 3 and "not set" in str(exc.value)
        for comp in range(c):
            eng.set_groups(0, comp, s["has_components"][:, comp][None, :])
        eng.set_weights(0, s["w"])
        with pytest.raises(EngineError) as exc:            # ... the source is still missing
            wgibbs.step(eng, 0, 0, 1, a2, u, alpha, ab, 1.0)
        assert exc.value.code == 3
        eng.set_source(0, wc.source_array(s["src"], c))
        assert raw_step(eng, 0, 0, 1, 1.0) == 0
        assert raw_step(eng, 1, 0, 1, 1.0) == 3            # the other slot holds nothing
        for i1, i2 in ((0, 0), (-1, 1), (0, c), (c, 0)):   # SBE_ERR_ARG: bad indices (the host layer is bypassed)
            assert raw_step(eng, 0, i1, i2, 1.0) == 1 and lib.sbe_wgibbs_pair_counts(eng._h, 0, i1, i2, ptr(cnt)) == 1
            assert b"two different indices" in lib.sbe_last_error(eng._h)
        for t in (0.0, -1.0, float("inf"), float("nan")):
            assert raw_step(eng, 0, 0, 1, t) == 1 and b"positive and finite" in lib.sbe_last_error(eng._h)
        assert raw_step(eng, 2, 0, 1, 1.0) == 1 and raw_step(eng, -1, 0, 1, 1.0) == 1
        assert raw_step(eng, 0, 0, 1, 1.0, a2_ptr=ct.c_void_p(None)) == 1 and b"null pointer" in lib.sbe_last_error(eng._h)
        assert lib.sbe_wgibbs_pair_counts(eng._h, 0, 0, 1, None) == 1
        assert raw_step(eng, 0, 0, 1, 1.0) == 0            # the engine is usable after every refusal
