"""The spatial posterior predictive check on the device (sbayes_amd.spatial, include/sbe_spatial.h) against
tests/_spatial_oracle.py on the cases of tests/_spatial_cases.py.  Every quantity is an integer: the observed arrays, every
optional per-replicate output and every accumulator EQUAL the oracle's; the planted cases have their closed forms; the reads are
byte-identical for any split of the replicates, any tile, with and without the optional outputs and after a reset; errors come in
the contract's order and change nothing; and spatial_check runs end to end on the recorded runs."""
from math import comb

import numpy as np
import pytest

from sbayes_amd import ppc, spatial
from sbayes_amd.engine import EngineError
from tests import _ppc_cases as ppc_cases
from tests import _spatial_cases as cases
from tests import _spatial_oracle as orc

pytestmark = pytest.mark.gpu
OBSERVED = tuple(f"{k}_obs" for k in orc.STATS)
FIELDS = OBSERVED + orc.ACCUMULATORS
REPS = tuple(f"{k}_rep" for k in orc.STATS)
ERR_ARG, ERR_STATE, ERR_DATA = 1, 3, 4
NA = orc.NA


def _bytes(res):
    return b"".join(np.ascontiguousarray(getattr(res, k)).tobytes() for k in FIELDS + ("total_rep",)) + str(res.n_replicates).encode()


def _equals(res, want, reps=REPS):
    for k in FIELDS + tuple(reps):
        got = getattr(res, k)
        assert got.shape == want[k].shape and np.array_equal(got, want[k]), k
    assert res.n_replicates == want["n_replicates"]
    for k in OBSERVED[:4] + ("f_greater", "i_less", "t_equal"):
        assert getattr(res, k).dtype == np.int32, k
    for k in ("total_obs", "f_sum", "i_sumsq", "total_rep"):
        assert getattr(res, k).dtype == np.int64, k


@pytest.fixture(scope="module")
def handle():
    h = spatial.SpatialHandle(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def device(handle):
    """name -> the device's result of the case with all replicates in one add call and every optional output kept; computed once."""
    done = {}

    def get(name):
        if name not in done:
            x, ns, band, b, y, _want = cases.case(name)
            handle.set_tile(0)
            handle.set_data(x, ns, band, b)
            handle.add(y, keep=True)
            done[name] = handle.result()
        return done[name]
    return get


@pytest.mark.parametrize("name", list(cases.CASES))
def test_a_case_equals_the_oracle(device, name):
    x, ns, band, b, y, want = cases.case(name)
    res = device(name)
    _equals(res, want)
    assert np.array_equal(res.local_agree_obs.sum(axis=1), 2 * res.total_obs)
    assert np.array_equal(res.local_agree_rep.sum(axis=2), 2 * res.total_rep)
    p = res.p_value()
    assert ((p >= 0) & (p <= 1)).all() and (res.f_equal >= 1).all() and (res.i_equal >= 1).all() and (res.t_equal >= 1).all()


def test_the_hand_case(handle):
    x, ns, band, b, y = cases.hand()
    handle.set_tile(0)
    handle.set_data(x, ns, band, b)
    handle.add(y, keep=True)
    res = handle.result()
    assert res.agree_obs.tolist() == [[2, 0], [0, 1]] and res.comparable_obs.tolist() == [[3, 1], [2, 1]]
    assert res.local_agree_obs.tolist() == [[1, 1, 1, 1], [1, 0, 1, 0]] and res.total_obs.tolist() == [2, 1]
    assert res.total_rep.tolist() == [[2, 1], [3, 3]] and res.f_greater.tolist() == [[1, 0], [1, 0]] and res.f_equal.tolist() == [[1, 2], [1, 2]]
    assert res.f_sumsq.tolist() == [[13, 0], [4, 2]] and res.p_value("total").tolist() == [0.75, 0.75] and res.p_value()[0].tolist() == [0.75, 0.5]


@pytest.mark.parametrize("n, f", [(1, 1), (2, 3), (65, 17), (130, 2)])
def test_one_state_on_the_complete_graph(handle, n, f):
    x, ns, band, b = cases.constant(n, f)
    handle.set_tile(0)
    handle.set_data(x, ns, band, b)
    handle.add(np.repeat(x[None], 3, axis=0))
    res = handle.result()
    assert (res.agree_obs == n * (n - 1) // 2).all() and np.array_equal(res.comparable_obs, res.agree_obs)
    assert (res.local_agree_obs == (n - 1) * f).all() and res.total_obs.tolist() == [f * n * (n - 1) // 2]
    # replicates equal to the data: ties everywhere
    assert (res.f_equal == 3).all() and (res.i_equal == 3).all() and (res.t_equal == 3).all() and not res.f_greater.any() and not res.i_less.any()
    assert np.array_equal(res.f_sum, 3 * res.agree_obs.astype(np.int64)) and np.array_equal(res.i_sumsq, 3 * res.local_agree_obs.astype(np.int64) ** 2)


@pytest.mark.parametrize("n, h", [(2, 1), (64, 1), (65, 32), (129, 64)])
def test_two_halves(handle, n, h):
    x, ns, band, b = cases.halves(n, h, 2)
    handle.set_tile(0)
    handle.set_data(x, ns, band, b)
    res = handle.result()
    assert (res.agree_obs[0] == comb(h, 2) + comb(n - h, 2)).all() and np.array_equal(res.comparable_obs[0], res.agree_obs[0])
    assert not res.agree_obs[1].any() and (res.comparable_obs[1] == h * (n - h)).all() and res.n_replicates == 0
    assert res.local_agree_obs[0].tolist() == [2 * (h - 1)] * h + [2 * (n - h - 1)] * (n - h) and not res.local_agree_obs[1].any()


@pytest.mark.parametrize("name", ["n2", "n64", "n65", "n129", "n257"])
def test_reads_do_not_depend_on_the_split_the_tile_or_the_outputs(device, name):
    x, ns, band, b, y, want = cases.case(name)
    ref = _bytes(device(name))
    t_n = y.shape[0]
    h = spatial.SpatialHandle(0)
    try:
        h.set_data(x, ns, band, b)
        for split in ((2, t_n - 2), (1,) * t_n):
            h.reset()
            at = 0
            for n in split:
                h.add(y[at:at + n])
                at += n
            assert _bytes(h.result()) == ref, split
        for tile, keep in ((1, ()), (2, ("comparable_rep",)), (5, ("local_comparable_rep", "agree_rep")), (cases.TILE - 1, ()), (cases.TILE, True),
                           (cases.TILE + 1, ("local_agree_rep",)), (32, ())):
            h.set_tile(tile)
            h.set_data(x, ns, band, b)                                     # (the observed arrays under this tile as well)
            h.add(y, keep=keep)
            res = h.result()
            assert _bytes(res) == ref, tile
            _equals(res, want, reps=tuple(keep) if keep is not True else REPS)
            assert all(getattr(res, k) is None for k in spatial.REP_OUTPUTS if keep is not True and k not in keep)
        h.set_tile(0)
        h.reset()
        got = h.result()
        assert not any(getattr(got, k).any() for k in orc.ACCUMULATORS) and got.n_replicates == 0 and got.total_rep.shape == (0, b)
        assert all(np.array_equal(getattr(got, k), want[k]) for k in OBSERVED)
        h.add(y)
        assert _bytes(h.result()) == ref
        with pytest.raises(EngineError, match=r"tile_features=33 out of range \[0, 32\]"):
            h.set_tile(33)
        with pytest.raises(EngineError, match="tile_features=-1 out of range"):
            h.set_tile(-1)
    finally:
        h.close()


def test_set_data_refuses_in_the_contracts_order_and_leaves_no_data():
    x, ns, band, b, y, _want = cases.case("n65")
    h = spatial.SpatialHandle(0)
    lib = h._lib
    try:
        def set_data(x=x, ns=ns, band=band, b=b, n=x.shape[0], f=x.shape[1]):
            x, ns, band = np.ascontiguousarray(x), np.ascontiguousarray(ns, dtype=np.int32), np.ascontiguousarray(band)
            return lib.sbe_spatial_set_data(h._h, x.ctypes.data, n, f, ns.ctypes.data, band.ctypes.data, b), h._last_error()

        bad_x, bad_ns, bad_band = np.array(x), np.array(ns), np.array(band)
        bad_x[3, 2], bad_x[60, 0] = ns[2], 200
        bad_ns[5] = 33
        bad_band[7, 9] = bad_band[9, 7] = b                                 # out of range (both ways), behind an asymmetric entry
        bad_band[2, 4] = (band[2, 4] + 1) % b
        bad_band[9, 9] = 77                                                  # (the diagonal is ignored)
        # arguments before data, codes before classes, a class out of range before an asymmetric one
        assert set_data(n=0)[0] == ERR_ARG and set_data(n=4097)[0] == ERR_ARG and set_data(f=0)[0] == ERR_ARG and set_data(f=4097)[0] == ERR_ARG
        code, msg = set_data(x=bad_x, ns=bad_ns, band=bad_band, b=9)
        assert code == ERR_ARG and "n_states[5]=33 out of range [1, 32]" in msg
        code, msg = set_data(x=bad_x, band=bad_band, b=9)
        assert code == ERR_ARG and "n_bands=9 out of range [1, 8]" in msg
        assert set_data(x=bad_x, band=bad_band, b=0)[0] == ERR_ARG
        code, msg = set_data(x=bad_x, band=bad_band)
        assert code == ERR_DATA and f"x[3][2]={int(ns[2])} is neither below n_states[2]={int(ns[2])} nor 255" in msg
        code, msg = set_data(band=bad_band)
        assert code == ERR_DATA and f"band[7][9]={b} is neither below n_bands={b} nor 255" in msg
        bad_band[7, 9] = bad_band[9, 7] = NA
        code, msg = set_data(band=bad_band)
        assert code == ERR_DATA and f"band[2][4]={int(bad_band[2, 4])} differs from band[4][2]={int(band[4, 2])}" in msg
        assert orc.check_band(bad_band, b) in msg                            # (the checker words the offence the same way)
        # a refused call leaves the handle without data, also after a good one
        h.set_data(x, ns, band, b)
        h.add(y[:1])
        assert set_data(band=bad_band)[0] == ERR_DATA
        out = np.zeros((1,) + x.shape, dtype=np.uint8)
        assert lib.sbe_spatial_add(h._h, 1, out.ctypes.data, None, None, None, None, None) == ERR_STATE and "needs the data" in h._last_error()
        assert lib.sbe_spatial_reset(h._h) == ERR_STATE
        with pytest.raises(EngineError, match="sbe_spatial_read needs the data"):
            h.result()
        bad_band[2, 4] = band[2, 4]
        h.set_data(x, ns, bad_band, b)                                       # junk on the diagonal alone is fine, and clears the accumulators
        assert h.result().n_replicates == 0 and not h.result().f_equal.any()
    finally:
        h.close()


def test_add_errors_leave_the_accumulators_alone(device):
    x, ns, band, b, y, _want = cases.case("n129")
    h = spatial.SpatialHandle(0)
    try:
        with pytest.raises(ValueError, match="no data yet"):
            h.add(y)
        h.set_data(x, ns, band, b)
        h.add(y[:2])
        before = _bytes(h.result())
        bad = np.array(y[2:4])
        bad[1, 100, 4] = ns[4]                                             # replicate 1 of the call, and a later offender behind it
        bad[1, 128, 0] = 200
        with pytest.raises(EngineError, match=rf"y_rep\[1\]\[100\]\[4\]={int(ns[4])} is neither below n_states\[4\] nor 255") as e:
            h.add(bad, keep=True)
        assert e.value.code == ERR_DATA and _bytes(h.result()) == before
        bad[0, 0, 32] = 254
        with pytest.raises(EngineError, match=r"y_rep\[0\]\[0\]\[32\]=254 is neither"):
            h.add(bad)
        assert _bytes(h.result()) == before
        h.add(y[2:])
        assert _bytes(h.result()) == _bytes(device("n129"))
        out = np.zeros((1,) + x.shape, dtype=np.uint8)
        none = (None,) * 5
        assert h._lib.sbe_spatial_add(h._h, -1, out.ctypes.data, *none) == ERR_ARG and "n=-1 is negative" in h._last_error()
        assert h._lib.sbe_spatial_add(h._h, 1, None, *none) == ERR_ARG and "y_rep" in h._last_error()
        assert h._lib.sbe_spatial_add(h._h, 0, None, *none) == 0
        # blocks beyond the staging limit: refused in C (split in Python)
        n = h.call_replicates() + 1
        assert n - 1 == spatial.MAX_STAGE_BYTES // spatial.replicate_bytes(129, 33, 3, 1)
        assert h._lib.sbe_spatial_add(h._h, n, out.ctypes.data, *none) == ERR_ARG and "exceed the 268435456 bytes one call holds" in h._last_error()
        assert _bytes(h.result()) == _bytes(device("n129"))
    finally:
        h.close()


def test_python_splits_blocks_beyond_the_staging_limit(device, monkeypatch):
    x, ns, band, b, y, _want = cases.case("n63")
    ref = device("n63")
    h = spatial.SpatialHandle(0)
    try:
        h.set_data(x, ns, band, b)
        monkeypatch.setattr(spatial, "MAX_STAGE_BYTES", 2 * spatial.replicate_bytes(63, 15, 4, 8) + 1)
        assert h.call_replicates() == 2
        h.add(y, keep=True)
        res = h.result()
        assert _bytes(res) == _bytes(ref) and all(np.array_equal(getattr(res, k), getattr(ref, k)) for k in spatial.REP_OUTPUTS)
        assert len(h._kept) == 3
    finally:
        h.close()


def test_more_replicates_than_the_sums_of_squares_hold_are_refused(device):
    """At 4096 objects and 3 features the handle holds 131136 replicates; no call can stage that many, so the refusal is reached
    through the argument: it comes before the staging limit's, and counts the replicates the handle already holds."""
    x, ns, band, b, y, _want = cases.case("n4096")
    assert device("n4096").n_replicates == 2                               # (the module's handle holds this case now)
    h = spatial.SpatialHandle(0)
    try:
        h.set_data(x, ns, band, b)
        cap = h.max_replicates()
        assert cap == 131136 == h._lib.sbe_spatial_max_replicates(4096, 3)
        none = (None,) * 5
        assert h._lib.sbe_spatial_add(h._h, cap + 1, y.ctypes.data, *none) == ERR_ARG
        assert "131137 replicates after 0 exceed the 131136" in h._last_error()
        assert h._lib.sbe_spatial_add(h._h, cap, y.ctypes.data, *none) == ERR_ARG and "bytes one call holds" in h._last_error()
        h.add(y)
        assert h._lib.sbe_spatial_add(h._h, cap - 1, y.ctypes.data, *none) == ERR_ARG
        assert "131135 replicates after 2 exceed the 131136" in h._last_error()
        assert h._lib.sbe_spatial_add(h._h, cap - 2, y.ctypes.data, *none) == ERR_ARG and "bytes one call holds" in h._last_error()
        assert _bytes(h.result()) == _bytes(device("n4096"))
    finally:
        h.close()


@pytest.mark.parametrize("r", [0, 1])
def test_spatial_check_on_a_recorded_run(r):
    case = ppc_cases.recorded(r)
    n = case["codes"].shape[0]
    rng = np.random.default_rng(40 + r)
    band, b = spatial.bands_from_costs(spatial.plane_distances(rng.random((n, 2))), n_bands=4 if r == 0 else None, knn=None if r == 0 else 6)
    res = spatial.spatial_check(**case, band=band, n_bands=b, burnin=0.1, seed=ppc_cases.SEED, keep=True, device=0)
    chk = ppc.posterior_predictive_check(**case, burnin=0.1, seed=ppc_cases.SEED, replicates=True, device=0)
    assert res.n_replicates == chk.n_samples == 54 and res.ppc.y_rep is None
    assert np.array_equal(res.ppc.dev_feature, chk.dev_feature) and np.array_equal(res.ppc.p_feature, chk.p_feature)
    n_states = np.full(36, case["tables"].shape[3], dtype=np.int32)
    want = orc.check(case["codes"], n_states, band, b, chk.y_rep)
    _equals(res, want)
    p = res.p_value()
    assert ((p >= 0) & (p <= 1)).all() and np.array_equal(res.mean("total"), want["total_rep"].mean(axis=0))
