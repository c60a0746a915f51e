"""k_psens_weights (sbayes_amd/csrc/sbe_psens.hip) over its range, device against checker: the cases of
tests/_psens_range_cases.py -- draw counts at the tail thresholds, with a tail longer than the workgroup, at the LDS limit and on
the global path by size; ties at the cutoff rank; delta from 1e-8 to 4; log ratios whose spread floors the cutoff, underflows
the weights, overflows the range or vanishes; unequal chains and 64 of them; the tail buffer's capacity at 2^20 draws.

Per vector: the flag and the kind of k (inf, NaN) equal, a finite k within orc.tol_k (1e-10 plus 8 times the checker's own
spread under a one-ulp probe, computed on the CPU from the checker alone: tests/test_psens_range_cpu.py), every weight within
WEIGHT_EPS of exp(the checker's log weight) and two subnormal steps, their sum, ess; the same bits on both paths and for any
split into chains; and the sums of the column kernel under these weights, zeros among them."""
import numpy as np
import pytest

from sbayes_amd import _handle, psens
from tests import _psens_oracle as orc
from tests import _psens_range_cases as rc
from tests.test_gpu_psens import WEIGHT_EPS, _bits, _compare

pytestmark = pytest.mark.gpu

WEIGHT_ATOL = 1e-323                     # two subnormal steps; what a weight may be where the checker's is exactly 0
SUM_TOL, ESS_RTOL = 1e-12, 1e-9
SWITCH_MAX_DRAWS = 50_000                # below it, every case runs again under set_global_path(True)


def _store(chains, capacity, piece=None):
    h = psens.PsensHandle()
    try:
        h.reset(len(chains), chains[0].shape[1], capacity)
        for chain, rows in enumerate(chains):
            step = piece or len(rows)
            for r0 in range(0, len(rows), step):
                h.append(chain, rows[r0:r0 + step])
    except BaseException:
        h.close()
        raise
    return h


def _weights(h, c, burn=None):
    return h.weights_from_components(c.columns, delta=c.delta, burnin=c.burn if burn is None else burn, weights=True)


def _same_bits(a, b):
    return all(_bits(x) == _bits(y) for x, y in zip(a, b))


def _check(got, ref, n, label):
    """Every output of a weights call against the checker's; nothing is left out of a comparison."""
    k, ess, vflag, w = got
    assert np.array_equal(vflag, ref.vflag), (label, vflag, ref.vflag)
    assert np.array_equal(np.isinf(k), np.isinf(ref.k)) and np.array_equal(np.isnan(k), np.isnan(ref.k)), (label, k, ref.k)
    assert np.array_equal(np.sign(k[np.isinf(k)]), np.sign(ref.k[np.isinf(k)])), (label, k)
    finite = np.isfinite(ref.k)
    err = np.abs(k[finite] - ref.k[finite])
    worst = float(np.max(err / ref.tol_k[finite])) if err.size else 0.0
    want = np.exp(ref.lws)
    normal = (w > 0.0) & (want >= np.finfo(np.float64).tiny)                 # (a subnormal weight has no relative accuracy to report)
    dlw = float(np.max(np.abs(np.log(w[normal]) - ref.lws[normal]))) if normal.any() else 0.0
    print(f"[psens-range] {label}: N = {n}, largest |k - checker| / tol_k = {worst:.3g} (largest tol_k {ref.tol_k.max():.3g}), "
          f"largest |log w - checker| over the normal weights = {dlw:.3g}, weights exactly 0 in the checker: {int(np.sum(want == 0.0))}")
    assert np.all(err <= ref.tol_k[finite]), (label, k, ref.k, ref.tol_k)
    assert w.shape == want.shape
    off = np.abs(w - want)
    allowed = WEIGHT_EPS * want + WEIGHT_ATOL
    assert np.all(off <= allowed), (label, np.argwhere(~(off <= allowed))[:5].tolist(), float(np.nanmax(off / allowed)))
    assert np.all(w[want == 0.0] <= WEIGHT_ATOL) and np.all(w >= 0.0), label
    assert np.all(np.abs(w.sum(axis=1) - 1.0) <= SUM_TOL), (label, w.sum(axis=1))
    assert np.allclose(ess, ref.ess, rtol=ESS_RTOL, atol=0.0), (label, ess, ref.ess)
    constant = (ref.vflag & orc.VFLAG_CONSTANT) != 0
    assert np.all(w[constant] == 1.0 / n) and np.all(k[constant] == np.inf) and np.all(ess[constant] == float(n)), label


@pytest.mark.parametrize("name", rc.NAMES)
def test_the_weights_over_their_range(name):
    c = rc.case(name)
    ref = rc.reference(c)
    n, v = len(rc.stacked(c)), 2 * len(c.columns)
    assert psens.lds_max_draws() == rc.LDS_MAX_DRAWS
    h = _store(c.chains, c.capacity, c.piece)
    try:
        got = _weights(h, c)
        assert h.last_shape()[:4] == (len(c.chains), n, v, rc.path_by_size(n))          # the path by size, no switch
        assert h.last_kernel_times()[0] > 0.0
        if n < SWITCH_MAX_DRAWS:
            h.set_global_path(True)
            again = _weights(h, c)
            assert h.last_shape()[:4] == (len(c.chains), n, v, "global")
            assert _same_bits(got, again), name
    finally:
        h.close()
    _check(got, ref, n, name)


@pytest.mark.parametrize("name", rc.CHAIN_CASES)
def test_chains_give_the_bits_of_one_chain_of_their_kept_draws(name):
    c = rc.case(name)
    outs = []
    for chains, burn, capacity, piece in ((c.chains, c.burn, c.capacity, c.piece), ([rc.stacked(c)], [0], None, None)):
        h = _store(chains, capacity or len(chains[0]), piece)
        try:
            outs.append(_weights(h, c, burn))
            assert h.last_shape()[:2] == (len(chains), len(rc.stacked(c)))
        finally:
            h.close()
    assert _same_bits(*outs), name


@pytest.mark.parametrize("name", rc.SUMS_CASES)
def test_the_sums_under_the_devices_own_weights(name):
    """compute() after the weights call: a tail above the workgroup, weights that are exactly 0 or tiny (the column kernel's
    Q > 0 ? log2(Q) : 0 branch under weights the device wrote itself), and 64 chains."""
    c = rc.case(name)
    x = rc.stacked(c)
    assert x.shape[1] == 2
    h = _store(c.chains, c.capacity, c.piece)
    try:
        _k, _ess, vflag, w = _weights(h, c)
        got = h.compute()
        assert h.last_shape()[:3] == (len(c.chains), len(x), 2)
    finally:
        h.close()
    if name == "spread_2000":
        assert np.all(np.sum(w == 0.0, axis=1) > 50)
    _compare(got, orc.table(x, w, vflag), len(x), name)


def test_ratios_that_overflow_are_refused_and_the_handle_goes_on():
    """x = 1e308 at delta = 4: finite, but (alpha - 1) x is +inf for alpha > 1.  SBE_ERR_ARG with the column's number, no weights
    left behind, and a valid call on the same handle afterwards gives what a fresh handle gives."""
    c = rc.overflow_case()
    h = _store(c.chains, c.capacity)
    try:
        with pytest.raises(_handle.EngineError, match=r"component column 1 holds a non-finite value, or its log ratios at delta=4 overflow") as info:
            h.weights_from_components(c.columns, delta=c.delta, burnin=0.0)
        assert info.value.code == 1                                          # SBE_ERR_ARG
        with pytest.raises(_handle.EngineError, match="no weights"):
            h.compute()
        after = h.weights_from_components([0], delta=c.delta, burnin=0.0, weights=True)
        sums = h.compute()
    finally:
        h.close()
    fresh = _store(c.chains, c.capacity)
    try:
        want = fresh.weights_from_components([0], delta=c.delta, burnin=0.0, weights=True)
        want_sums = fresh.compute()
    finally:
        fresh.close()
    assert _same_bits(after, want) and _bits(sums.js) == _bits(want_sums.js) and np.array_equal(sums.flag, want_sums.flag)
    lws, ks, ess, flags = orc.component_weights(rc.stacked(c), [0], c.delta)
    assert np.array_equal(after[2], flags) and np.allclose(after[3], np.exp(lws), rtol=WEIGHT_EPS, atol=WEIGHT_ATOL)


def _long(n):
    c = rc.long_case(n)
    ref = rc.reference(c)
    assert orc.tail_anatomy(rc.vectors(c)[0])[:2] == (orc.tail_count(n), orc.tail_count(n))
    h = _store(c.chains, c.capacity)
    try:
        got = _weights(h, c)
        assert h.last_shape()[:4] == (1, n, 2, "global")
        ms = h.last_kernel_times()[0]
    finally:
        h.close()
    print(f"[psens-range] long_{n}: the weights kernel took {ms:.1f} ms (2 vectors, tail {orc.tail_count(n)}, "
          f"{30 + int(orc.tail_count(n) ** 0.5)} candidates)")
    _check(got, ref, n, c.name)


def test_a_tail_of_more_than_a_thousand_at_2_17_draws():
    """N = 2^17 after 1000 burnt rows: 512 keys a thread in the network, a tail of 1087 (five trips of the workgroup), 62
    candidates."""
    _long(rc.CAPACITY_PROBE_DRAWS)


def test_the_tail_buffer_and_the_candidates_at_capacity():
    """N = 2^20 after 1000 burnt rows, the most a call takes: the only size with a tail of kPsensMaxTail = 3072 (twelve trips of the
    workgroup over the exceedances' scratch) and 85 candidates of kPsensMaxM = 96.  The weights kernel was timed at 9.7 ms at
    2^17 draws, which projects to 0.11 s here by the network's keys and stages (profiles/psens/README.md has what it took)."""
    assert orc.tail_count(rc.CAPACITY_DRAWS) == rc.MAX_TAIL
    _long(rc.CAPACITY_DRAWS)
