"""The float64 restatement of the Gibbs weights step (tests/_wgibbs_oracle.py) against what the reference's own
GibbsSampleWeights._propose computed (tests/golden/wgibbs.npz), the identity of its beta draw, and hand-checkable cases."""
import numpy as np
import pytest
from scipy import stats

from tests import _wgibbs_cases as wc
from tests import _wgibbs_oracle as worc


@pytest.mark.parametrize("tag", wc.CASES)
def test_oracle_equals_the_recorded_reference(tag):
    """Counts and w_new bit-exact; |log p_ref - log p_oracle| <= (N + 1) 2^-24 S_lh / T + 1e-12 (the worst case of the
    reference's serial float32 sums of float32 logs: loose on purpose); every recorded decision equal, and none inside the
    device band (the fixture's tie condition)."""
    case = wc.load(tag)
    n, f, c = case["shape"]
    t = case["prior_temperature"]
    assert case["proposals"]
    for k, p in enumerate(case["proposals"]):
        counts = worc.pair_counts(p["patterns"], p["pid"], p["src"], case["na"], p["i1"], p["i2"])
        assert np.array_equal(counts, p["counts"]), (tag, k)
        assert np.array_equal(worc.beta_parameters(counts, case["concentration_array"], p["i1"], p["i2"], t), p["beta_ab"])
        w_out, accept, terms, w_new = wc.oracle_step(case, p)
        assert w_new.dtype == np.float32 and w_new.tobytes() == p["w_new"].tobytes(), (tag, k)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            log_p_ref = ((p["log_lh_new"] + p["log_prior_new"]) - (p["log_lh_old"] + p["log_prior_old"])
                         + p["log_q_back"] - p["log_q"]) / t
            assert np.array_equal(np.exp(log_p_ref), p["p_accept"], equal_nan=True)
        finite = np.isfinite(log_p_ref) & np.isfinite(terms["log_p"])
        assert np.array_equal(np.isnan(log_p_ref), np.isnan(terms["log_p"]))
        err = np.abs(log_p_ref - terms["log_p"])[finite]
        assert (err <= worc.reference_bound(terms, n, t)[finite]).all(), (tag, k, err.max())
        assert np.array_equal(accept, p["accept"]), (tag, k)
        assert w_out.tobytes() == p["w_out"].tobytes(), (tag, k)
        assert (worc.log_margin(p["u"], terms["log_p"]) > worc.device_band(terms, t)).all(), (tag, k)
        assert p["version"][1] == p["version"][0] + 2


def test_the_fixture_covers_what_its_case_names_say():
    kinds = {tag: wc.load(tag) for tag in wc.CASES}
    assert kinds["south_america_mc3"]["prior_temperature"] == 1.5
    assert kinds["south_america_symdir"]["prior_type"] == "symmetric_dirichlet" and (kinds["south_america_symdir"]["alpha"] < 1).all()
    assert kinds["south_america_jeffreys"]["prior_type"] == "jeffreys" and (kinds["south_america_jeffreys"]["alpha"] == 0.5).all()
    assert kinds["south_america_bbs"]["prior_type"] == "BBS"
    assert kinds["headline"]["shape"] == (1000, 200, 2) and kinds["cfg1"]["shape"] == (50, 30, 2)
    rejected = sum(int((~p["accept"]).sum()) for c in kinds.values() for p in c["proposals"])
    accepted = sum(int(p["accept"].sum()) for c in kinds.values() for p in c["proposals"])
    assert rejected >= 100 and accepted >= 100              # both decisions are well represented


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_frozen_beta_rvs_is_np_random_beta_on_the_same_stream(seed):
    """stats.beta(a, b).rvs() -- what the reference draws a2 with -- is np.random.beta(a, b, size=F) on the global stream,
    bit for bit, and leaves the stream in the same state."""
    rng = np.random.default_rng(seed)
    a, b = 1 + rng.random(37) * 50, 1 + rng.random(37) * 50
    np.random.seed(100 + seed)
    want = stats.beta(a, b).rvs()
    state_ref = np.random.get_state()
    np.random.seed(100 + seed)
    got = np.random.beta(a, b, size=37)
    state_new = np.random.get_state()
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    assert all(np.array_equal(x, y) for x, y in zip(state_ref, state_new))


def test_log_ratio_matches_scipy_density_differences():
    """The cancellation argument: the ratio without ln B(alpha) and betaln equals the differences of SciPy's full
    log-densities to rounding."""
    rng = np.random.default_rng(5)
    f, c = 40, 4
    w = rng.dirichlet(np.ones(c), f).astype(np.float32)
    alpha = rng.random((f, c)) * 2 + 0.2
    ab = 1 + rng.random((f, 2)) * 30
    a2 = rng.beta(ab[:, 0], ab[:, 1])
    w_new, a2_old = worc.propose_weights(w, 1, 3, a2)
    patterns, pid = np.ones((1, c), dtype=bool), np.zeros(0, dtype=np.int64)
    terms = worc.log_ratio(w, w_new, a2_old, patterns, pid, np.zeros((0, f), dtype=np.int16), np.zeros((0, f), dtype=bool), a2,
                           alpha, ab, 1.0)
    assert np.all(terms["d_lh"] == 0)
    want_prior = np.array([stats.dirichlet._logpdf(w_new[i], alpha[i]) - stats.dirichlet._logpdf(w[i], alpha[i]) for i in range(f)])
    d = stats.beta(ab[:, 0], ab[:, 1])
    want_q = d.logpdf(a2_old.astype(np.float64)) - d.logpdf(a2)
    np.testing.assert_allclose(terms["d_prior"], want_prior, rtol=0, atol=1e-12)
    np.testing.assert_allclose(terms["d_q"], want_q, rtol=0, atol=1e-12)


def _tiny(rng, n=12, f=5, c=3):
    hc = rng.random((n, c)) < 0.7
    hc[:, 1] = True
    src = np.array([[rng.choice(np.flatnonzero(hc[i])) for _ in range(f)] for i in range(n)], dtype=np.int16)
    na = rng.random((n, f)) < 0.2
    src[na] = -1
    patterns, pid = np.unique(hc, axis=0, return_inverse=True)
    w = rng.dirichlet(np.ones(c), f).astype(np.float32)
    return w, patterns, np.asarray(pid).reshape(-1), src, na


def test_uniform_prior_has_no_prior_term():
    rng = np.random.default_rng(1)
    w, patterns, pid, src, na = _tiny(rng)
    a2 = rng.random(w.shape[0])
    w_new, a2_old = worc.propose_weights(w, 0, 2, a2)
    terms = worc.log_ratio(w, w_new, a2_old, patterns, pid, src, na, a2, np.ones(w.shape), np.full((w.shape[0], 2), 3.0), 1.0)
    assert np.all(terms["d_prior"] == 0.0)
    w0 = w.copy()
    w0[:, 1] = 0                                            # alpha == 1: 0 whatever w is (xlogy)
    assert np.all(worc.log_ratio(w0, w_new, a2_old, patterns, pid, src, na, a2, np.ones(w.shape), np.full((w.shape[0], 2), 3.0),
                                 1.0)["d_prior"] == 0.0)


def test_proposing_the_current_split_gives_log_p_zero():
    rng = np.random.default_rng(2)
    _w, patterns, pid, src, na = _tiny(rng)
    # weights on a dyadic grid (multiples of 1/8, rows summing to 1, a2_old a multiple of 1/4): w02, a2_old and the two
    # products are exact, so proposing a2 = a2_old proposes the current row, and every term of the ratio is exactly zero
    w = np.array([[2, 4, 2], [1, 4, 3], [3, 4, 1], [2, 4, 2], [1, 4, 3]], dtype=np.float32) / 8
    a2_old = (w[:, 2] / (w[:, 0] + w[:, 2])).astype(np.float64)
    w_new, a2o = worc.propose_weights(w, 0, 2, a2_old)
    assert np.array_equal(a2o.astype(np.float64), a2_old) and np.array_equal(w_new, w)
    terms = worc.log_ratio(w, w_new, a2o, patterns, pid, src, na, a2_old, np.full(w.shape, 0.5), np.full((5, 2), 7.0), 1.3)
    assert np.all(terms["log_p"] == 0.0)
    assert worc.decide(np.full(5, 0.999, dtype=np.float32), terms["log_p"]).all()


def test_nan_rejects_and_keeps_the_old_row():
    rng = np.random.default_rng(3)
    w, patterns, pid, src, na = _tiny(rng)
    src[0, 0] = -1
    na[0, 0] = False                                        # an observation without a source component: log 0 - log 0
    f = w.shape[0]
    a2 = rng.random(f)
    u = np.zeros(f, dtype=np.float32)                       # u = 0 accepts whatever p > 0 is
    w_out, accept, terms, w_new = worc.step(w, patterns, pid, src, na, 0, 1, a2, u, np.ones(w.shape), np.full((f, 2), 2.0), 1.0)
    assert np.isnan(terms["log_p"][0]) and not accept[0] and np.array_equal(w_out[0], w[0])
    assert accept[1:].all() and np.array_equal(w_out[1:], w_new[1:])
    assert not worc.decide(np.float32(0.0), np.nan) and worc.decide(np.float32(0.0), -800.0) == (np.exp(-800.0) > 0)
