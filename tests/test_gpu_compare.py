"""sbayes_amd.compare on the device against the host restatement (tests/_compare_oracle.py).  The shapes sit at the edges of
the kernels' chunks, waves and runs (imported from the module); the tolerances rest on the summation rule of
include/sbe_compare.h: no accumulator adds more than RUN = 1024 terms in sequence, so a sum of same-signed terms is within
about (1024 + 40) 2^-53 = 1.2e-13 of the exact one, relative."""
import math
from functools import lru_cache

import numpy as np
import pytest

from sbayes_amd import compare, elpd
from sbayes_amd._handle import EngineError
from sbayes_amd.compare import BLOCK, BOOT_CHUNK, CHUNK, RUN
from tests import _compare_oracle as co

pytestmark = pytest.mark.gpu

TOL = 1e-8
LONG = RUN * BLOCK + 5                                   # above the 1024-term run length times the block size
# (N, M): every N of the list with the M in turn, 32 models at a small N and behind a chunk edge
SHAPES = [(1, 1), (2, 2), (63, 3), (64, 8), (65, 32), (CHUNK - 1, 2), (CHUNK, 3), (CHUNK + 1, 32), (2 * CHUNK + 3, 8), (LONG, 3)]


@pytest.fixture(scope="module")
def handle():
    h = compare.CompareHandle()
    yield h
    h.close()


@lru_cache(maxsize=None)
def values(n, m):
    """Seeded negative gamma draws around -2 (read-only: the tests share them)."""
    x = co.gamma_values(7000 + n + 13 * m, n, m)
    x.setflags(write=False)
    return x


@lru_cache(maxsize=None)
def tiny_likelihoods(n=CHUNK + 1, m=3):
    """Logs of float32 likelihoods near the smallest normal (about -700 .. -690) mixed with exact 0.0."""
    rng = np.random.default_rng(99)
    x = np.where(rng.random((n, m)) < 0.5, 0.0, -700.0 + 10.0 * rng.random((n, m)))
    x.setflags(write=False)
    return x


def fill(h, x):
    h.reset(x.shape[1], x.shape[0])
    for k in range(x.shape[1]):
        h.set_model(k, x[:, k])


def check_moments(got, got_root, want, want_root, terms, what):
    bound = 1e-12 * np.abs(terms).sum(axis=0)
    print(f"{what}: max |sum error| / bound = {np.max(np.abs(got - want) / np.maximum(bound, 1e-300)):.3g}, "
          f"max relative root error = {np.max(np.abs(got_root - want_root) / np.maximum(want_root, 1e-300)):.3g}")
    assert np.all(np.abs(got - want) <= bound), (what, got - want, bound)
    assert np.all(np.abs(got_root - want_root) <= 1e-10 * want_root), (what, got_root - want_root)


@pytest.mark.parametrize("n,m", SHAPES + [("tiny", 3)])
def test_totals_and_differences_meet_the_fsum_oracle(handle, n, m):
    x = tiny_likelihoods() if n == "tiny" else values(n, m)
    fill(handle, x)
    elpd_k, se = handle.totals()
    assert handle.last_kernel_ms() > 0.0
    want, want_se = co.totals(x)
    check_moments(elpd_k, se, want, want_se, x, f"totals N={n} M={m}")
    top = int(co.rank(want)[0])
    assert int(co.rank(elpd_k)[0]) == top
    for ref in {top, m - 1}:
        diff, dse = handle.differences(ref)
        want_diff, want_dse = co.differences(x, ref)
        check_moments(diff, dse, want_diff, want_dse, x[:, [ref]] - x, f"differences N={n} M={m} ref={ref}")
        assert diff[ref] == 0.0 and dse[ref] == 0.0
    again = handle.totals()
    assert np.array_equal(again[0], elpd_k) and np.array_equal(again[1], se)        # bit-identical from call to call


def check_stacking(x, result, tol, what):
    """The properties every stacking result has: the simplex, the reported gap against the gap recomputed on the host from the
    returned weights over the full data, and convergence as reported."""
    w, gap, updates, converged = result
    host_gap = co.gap(x, w)
    print(f"{what}: gap device {gap!r} host {host_gap!r} after {updates} updates, weights sum - 1 = {w.sum() - 1.0:.3g}")
    assert w.shape == (x.shape[1],) and np.all(w >= 0.0) and abs(math.fsum(w) - 1.0) <= 1e-12
    assert abs(gap - host_gap) <= 1e-12
    assert converged == (gap <= tol)
    return host_gap


@pytest.mark.parametrize("n,m", SHAPES[:-1] + [("tiny", 3)])
def test_stacking_converges_to_the_gap_it_reports(handle, n, m):
    x = tiny_likelihoods() if n == "tiny" else values(n, m)
    fill(handle, x)
    result = handle.stacking(tol=TOL)
    host_gap = check_stacking(x, result, TOL, f"stacking N={n} M={m}")
    assert result[3] and host_gap <= TOL + 1e-12
    w_oracle, gap_oracle, _updates, converged = co.stacking(x, tol=TOL, exact=False)
    assert converged and gap_oracle <= TOL
    f_device, f_oracle = co.objective(x, result[0]), co.objective(x, w_oracle)
    print(f"  f device {f_device!r} oracle {f_oracle!r}")
    assert f_device >= f_oracle - 1e-8
    again = handle.stacking(tol=TOL)                     # (on the p image the first call built)
    assert np.array_equal(again[0], result[0]) and again[1:] == result[1:]


@pytest.mark.parametrize("n1,n2,p,q", [(700, 300, 0.6, 0.2), (100, 900, 0.6, 0.2), (LONG - 9 * LONG // 20, 9 * LONG // 20, 0.5, 0.25)])
def test_stacking_meets_the_planted_two_model_optimum(handle, n1, n2, p, q):
    x, w0 = co.planted(n1, n2, p, q)
    fill(handle, x)
    result = handle.stacking(tol=TOL)
    host_gap = check_stacking(x, result, TOL, f"planted {n1}+{n2}")
    assert result[3] and host_gap <= TOL + 1e-12
    # along w_0 the objective has f'' <= -c, c = ((p - q) / max(p, q))^2: both denominators w p + (1 - w) q and w q + (1 - w) p are at
    # most max(p, q).  With f'(w*) (w - w*) <= 0 at the optimum (interior or clipped): (c / 2) (w_0 - w_0*)^2 <= f* - f(w) <= gap
    c = ((p - q) / max(p, q)) ** 2
    bound = math.sqrt(2 * host_gap / c) + 1e-12
    print(f"  w_0 device {result[0][0]!r} planted {w0!r} bound {bound:.3g}")
    assert abs(result[0][0] - w0) <= bound
    assert co.objective(x, result[0]) >= co.objective(x, np.array([w0, 1.0 - w0])) - 1e-8       # (the closed form is this case's oracle)


def test_stacking_that_runs_out_of_updates_reports_the_true_gap(handle):
    x = values(CHUNK + 1, 32)
    fill(handle, x)
    result = handle.stacking(tol=TOL, max_iter=3)
    host_gap = check_stacking(x, result, TOL, "max_iter=3")
    assert result[2] == 3 and not result[3] and host_gap > TOL
    just_over = handle.stacking(tol=TOL, max_iter=compare.CHECK_EVERY + 1)                   # one evaluation behind a read of the gap
    assert just_over[2] == compare.CHECK_EVERY + 1 and not just_over[3]
    check_stacking(x, just_over, TOL, "max_iter=R+1")


def test_stacking_follows_the_store(handle):
    """The p image belongs to one generation of the store: a model set anew is seen by the next call."""
    x = np.array(values(CHUNK - 1, 2))
    fill(handle, x)
    first = handle.stacking(tol=TOL)
    x[:, 0] = values(CHUNK - 1, 3)[:, 2]
    handle.set_model(0, x[:, 0])
    second = handle.stacking(tol=TOL)
    check_stacking(x, second, TOL, "after set_model")
    assert second[3] and not np.array_equal(first[0], second[0])


# (N, M, B): the lists of N, M and B with BOOT_CHUNK as the chunk, M = 9 and 17 for the 32-accumulator kernel's models behind M, and one N whose
# chunk partials exceed one run
BOOT_SHAPES = [(1, 1, 1), (2, 2, 63), (63, 3, 64), (64, 8, 65), (65, 32, 130), (BOOT_CHUNK - 1, 2, 65), (BOOT_CHUNK, 3, 64), (BOOT_CHUNK + 1, 32, 63),
               (2 * BOOT_CHUNK + 3, 8, 130), (BOOT_CHUNK + 1, 9, 65), (BOOT_CHUNK - 1, 17, 64), (CHUNK + 1, 2, 1), (RUN * BOOT_CHUNK + 7, 2, 1)]


def check_bootstrap(x, seed, b, got, what):
    weights, se, z = got
    want_w, want_se, want_z, _w_b, bound = co.bootstrap(x, seed, b)
    dz = 1e-12 * bound
    print(f"{what}: max |z error| / bound = {np.max(np.abs(z - want_z) / dz):.3g}, max |weight error| = {np.max(np.abs(weights - want_w)):.3g} "
          f"(allowed {2 * dz.max():.3g}), max relative se error = {np.max(np.abs(se - want_se) / np.maximum(want_se, 1e-300)):.3g}")
    assert z.shape == (b, x.shape[1]) and np.all(np.abs(z - want_z) <= dz), what
    assert np.all(np.abs(weights - want_w) <= 2 * dz.max()), what
    assert np.all(np.abs(se - want_se) <= 1e-9 * want_se), what


@pytest.mark.parametrize("n,m,b", BOOT_SHAPES + [("tiny", 3, 65)])
def test_bootstrap_meets_the_oracle_draw_for_draw(handle, n, m, b):
    x = tiny_likelihoods() if n == "tiny" else values(n, m)
    fill(handle, x)
    seed = 0x1234_5678_9ABC_DEF0 + b
    got = handle.bootstrap(seed, b, return_z=True)
    assert handle.last_kernel_ms() > 0.0
    check_bootstrap(x, seed, b, got, f"bootstrap N={n} M={m} B={b}")
    weights, se = handle.bootstrap(seed, b)                                     # (z_out NULL)
    assert np.array_equal(weights, got[0]) and np.array_equal(se, got[1])


def test_bootstrap_is_reproducible_and_independent_of_the_batch(handle):
    x = values(2 * BOOT_CHUNK + 3, 8)
    fill(handle, x)
    first = handle.bootstrap(11, 130, return_z=True)
    second = handle.bootstrap(11, 130, return_z=True)
    assert all(np.array_equal(a, b) for a, b in zip(first, second))
    other = handle.bootstrap(12, 130, return_z=True)
    assert not np.array_equal(first[2], other[2]) and not np.array_equal(first[0], other[0])
    handle.set_bootstrap_batch(64)                                              # three batches: 64 + 64 + 2 replicates
    try:
        batched = handle.bootstrap(11, 130, return_z=True)
    finally:
        handle.set_bootstrap_batch(0)
    assert all(np.array_equal(a, b) for a, b in zip(first, batched))
    with pytest.raises(EngineError, match="not a multiple of 64"):
        handle.set_bootstrap_batch(100)


def test_bootstrap_of_identical_columns_is_uniform(handle):
    x = np.repeat(values(300, 1), 4, axis=1)
    fill(handle, x)
    weights, se, z = handle.bootstrap(5, 65, return_z=True)
    assert np.array_equal(weights, np.full(4, 0.25)) and np.all(se == se[0]) and se[0] > 0 and np.all(z == z[:, [0]])


@lru_cache(maxsize=None)
def three_runs():
    """Three synthetic likelihood matrices (float32 [S, columns]) of falling quality, through psis_loo."""
    rng = np.random.default_rng(2718)
    s, cols = 40, 300
    base = rng.normal(-1.2, 0.5, cols)
    out = {}
    for name, shift in (("K2", -0.15), ("K3", 0.0), ("K4", -0.05)):
        ll = base[None, :] + shift * rng.random(cols)[None, :] + 0.05 * rng.standard_normal((s, cols))
        out[name] = elpd.psis_loo(np.exp(ll).astype(np.float32), na_values=np.zeros(cols, bool), burnin=0.0)
    return out


def test_compare_end_to_end_on_three_runs():
    loos = three_runs()
    res = compare.compare(loos, method="stacking")
    by_elpd = sorted(loos, key=lambda name: -loos[name].elpd_loo)
    assert res.names == by_elpd == ["K3", "K4", "K2"] and list(res.rank) == [0, 1, 2] and list(res.order) == [1, 2, 0]
    assert res.method == "stacking" and res.criterion == "loo" and res.scale == "log" and res.converged and 0.0 <= res.gap <= TOL
    assert res.elpd_diff[0] == 0.0 and res.dse[0] == 0.0 and np.all(res.elpd_diff[1:] > 0) and np.all(res.dse[1:] > 0)
    x = np.stack([loos[name].loo_i for name in loos], axis=1)
    want, want_se = co.totals(x)
    assert np.allclose(res.elpd, want[res.order], rtol=1e-12) and np.allclose(res.se, want_se[res.order], rtol=1e-10)
    assert np.allclose(res.elpd, [loos[name].elpd_loo for name in res.names], rtol=1e-12)
    assert np.allclose(res.p, [loos[name].p_loo for name in res.names], rtol=0, atol=0)
    assert abs(res.weight.sum() - 1.0) <= 1e-12 and abs(co.gap(x, res.weight[np.argsort(res.order)]) - res.gap) <= 1e-12
    lines = res.text().splitlines()
    assert lines[0] == "model\trank\telpd_loo\tp_loo\telpd_diff\tweight\tse\tdse\twarning\tscale" and len(lines) == 4
    assert [line.split("\t")[0] for line in lines[1:]] == ["K3", "K4", "K2"]
    top = lines[1].split("\t")
    assert top[1] == "0" and top[4] == "0" and top[7] == "0" and top[9] == "log" and float(top[2]) == float(f"{res.elpd[0]:.10g}")
    plain = compare.compare(loos, method="pseudo-bma")
    assert plain.names == res.names and np.allclose(plain.weight, co.pseudo_bma(want)[plain.order], rtol=1e-10) and np.isnan(plain.gap)
    boot = compare.compare(loos, method="bb-pseudo-bma", b_samples=65, seed=3)
    want_w, want_bse, _z, _w_b, bound = co.bootstrap(x, 3, 65)
    assert boot.names == res.names and np.all(np.abs(boot.weight - want_w[boot.order]) <= 2e-12 * bound.max())
    assert np.allclose(boot.se, want_bse[boot.order], rtol=1e-9) and np.array_equal(boot.elpd_diff, res.elpd_diff)
    vectors = compare.compare({name: loos[name].loo_i for name in loos})       # bare vectors: no p column
    assert vectors.names == res.names and vectors.criterion == "elpd" and np.all(np.isnan(vectors.p)) and np.array_equal(vectors.weight, res.weight)


def test_a_value_that_is_not_finite_is_refused_by_the_device_naming_the_model(handle):
    x = np.array(values(CHUNK + 1, 3))
    fill(handle, x)
    bad = x[:, 1].copy()
    bad[CHUNK - 7] = np.nan
    bad[CHUNK] = np.inf
    with pytest.raises(EngineError, match=rf"model 1: x\[{CHUNK - 7}\]=nan is not finite") as err:
        handle.set_model(1, bad)
    assert err.value.code == 4                            # SBE_ERR_DATA
    for call in (handle.totals, lambda: handle.differences(0), handle.stacking, handle.bootstrap):
        with pytest.raises(EngineError, match="model 1 has not been set since the last reset") as err:
            call()
        assert err.value.code == 3                        # SBE_ERR_STATE
    handle.set_model(1, x[:, 1])
    want, _se = co.totals(x)
    assert np.all(np.abs(handle.totals()[0] - want) <= 1e-12 * np.abs(x).sum(axis=0))
    handle.reset(2, 10)
    with pytest.raises(EngineError, match="model 0 has not been set"):
        handle.totals()
