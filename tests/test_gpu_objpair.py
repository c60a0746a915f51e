"""The object-pair posterior predictive check on the device (sbayes_amd.objpair, include/sbe_objpair.h) against
tests/_objpair_oracle.py on the cases of tests/_objpair_cases.py.  Every quantity is an integer: the observed counts, the
replicates' own counts and every accumulator EQUAL the checker's; the reads are byte-identical for any split of the replicates,
any launch-tile setting, with and without agree_rep and after a reset; the accumulator is exact at the largest count and on the
longest contraction axis; refusals name the offender and change nothing; and object_pair_check runs end to end on the recorded
runs, where it equals the checker on the posterior predictive check's replicates and adds up to the spatial check's counts."""
import numpy as np
import pytest

from sbayes_amd import objpair, ppc, spatial
from sbayes_amd.engine import EngineError
from tests import _objpair_cases as cases
from tests import _objpair_oracle as orc
from tests import _predict_cases as recorded_cases

pytestmark = pytest.mark.gpu
FIELDS = {"observed": "agree_obs", "comparable": "comparable_obs", **{k: k for k in orc.ACCUMULATORS}}
ERR_ARG, ERR_STATE, ERR_DATA = 1, 3, 4
SEED = 2201
NA = orc.NA


def _bytes(res):
    return b"".join(np.ascontiguousarray(getattr(res, k)).tobytes() for k in FIELDS) + str(res.n_replicates).encode()


def _equals(res, want, n=None):
    """res against the checker's result `want`, or against the checker on the first n replicates of the same case."""
    for k, name in FIELDS.items():
        got = getattr(res, k)
        assert got.shape == want[name].shape and np.array_equal(got, want[name]), k
        assert got.dtype == (np.int64 if k in ("sum", "sumsq") else np.int32), k
    assert res.n_replicates == want["n_replicates"]
    if res.agree_rep is not None:
        assert res.agree_rep.dtype == np.int32 and res.agree_rep.shape == want["agree_rep"].shape and np.array_equal(res.agree_rep, want["agree_rep"])


@pytest.fixture(scope="module")
def handle():
    h = objpair.ObjPairHandle(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def device(handle):
    """name -> the device's result of the case with all replicates in one add call and agree_rep kept; computed once."""
    done = {}

    def get(name):
        if name not in done:
            x, ns, y, _want = cases.case(name)
            handle.set_launch_tiles(0)
            handle.set_data(x, ns)
            handle.add(y, agree_rep=True)
            done[name] = handle.result(), handle.last_shape()
        return done[name][0]
    get.shape = lambda name: (get(name), done[name][1])[1]
    return get


@pytest.mark.parametrize("name", list(cases.CASES))
def test_a_case_equals_the_checker(device, name):
    x, ns, y, want = cases.case(name)
    res = device(name)
    _equals(res, want)
    n = x.shape[0]
    tiles = -(-n // 32)
    assert device.shape(name) == (orc.elements(ns)[1], tiles * (tiles + 1) // 2, 1)              # (one launch holds every tile pair)
    off = ~np.eye(n, dtype=bool)
    p = res.p_value()
    assert ((p[off] >= 0) & (p[off] <= 1)).all() and np.isnan(np.diag(p)).all() and (res.n_equal[off] >= 1).all()
    for k in FIELDS:
        assert not np.diag(getattr(res, k)).any(), k


def test_the_hand_case(handle):
    x, ns, y = cases.hand()
    handle.set_launch_tiles(0)
    handle.set_data(x, ns)
    rep = handle.add(y, agree_rep=True)
    res = handle.result()
    assert res.observed.tolist() == [[0, 2, 2], [2, 0, 1], [2, 1, 0]] and res.comparable.tolist() == [[0, 2, 3], [2, 0, 2], [3, 2, 0]]
    assert rep[1].tolist() == [[0, 2, 3], [2, 0, 2], [3, 2, 0]] and rep[2].tolist() == [[0, 1, 2], [1, 0, 2], [2, 2, 0]]
    assert res.n_greater.tolist() == [[0, 0, 1], [0, 0, 2], [1, 2, 0]] and res.n_equal.tolist() == [[0, 2, 2], [2, 0, 1], [2, 1, 0]]
    assert res.n_less.tolist() == [[0, 1, 0], [1, 0, 0], [0, 0, 0]] and res.sum.tolist() == [[0, 5, 7], [5, 0, 5], [7, 5, 0]]
    assert res.sumsq.tolist() == [[0, 9, 17], [9, 0, 9], [17, 9, 0]] and res.p_value()[0, 1] == 1 / 3 and res.n_replicates == 3


@pytest.mark.parametrize("name", ["n2", "n32", "n33", "n65", "n97"])
def test_reads_do_not_depend_on_the_split_the_launch_tiles_or_the_output(device, name):
    x, ns, y, want = cases.case(name)
    ref = _bytes(device(name))
    n_obj = x.shape[0]
    tiles = -(-n_obj // 32)
    h = objpair.ObjPairHandle(0)
    try:
        h.set_data(x, ns)
        for split in ((1, 4), (2, 3), (1,) * 5, (0, 5, 0)):
            h.reset()
            at = 0
            for n in split:
                h.add(y[at:at + n])
                at += n
            res = h.result()
            assert _bytes(res) == ref and res.agree_rep is None, split
        # n = 0, 1 and 5 replicates against the checker on as many
        for n in (0, 1):
            h.reset()
            h.add(y[:n], agree_rep=True)
            _equals(h.result(), orc.check(x, ns, y[:n]))
        h.reset()
        h.add(x[None])                                                       # a replicate equal to the data ties everywhere
        res = h.result()
        off = ~np.eye(n_obj, dtype=bool)
        assert (res.n_equal[off] == 1).all() and not res.n_greater.any() and not res.n_less.any() and not np.diag(res.n_equal).any()
        for launch, keep in ((1, False), (1, True), (2, False), (0, True)):
            h.set_launch_tiles(launch)
            h.set_data(x, ns)                                              # (the observed counts under this setting as well)
            if launch:
                assert h.last_shape() == (orc.elements(ns)[1], tiles * (tiles + 1) // 2, 2 * -(-(tiles * (tiles + 1) // 2) // launch))
            h.add(y, agree_rep=keep)
            if launch:
                assert h.last_shape()[2] == -(-(tiles * (tiles + 1) // 2) // launch)
            res = h.result()
            assert _bytes(res) == ref, launch
            _equals(res, want)
            assert (res.agree_rep is not None) == keep
        h.reset()
        got = h.result()
        assert not any(getattr(got, k).any() for k in orc.ACCUMULATORS) and got.n_replicates == 0
        assert np.array_equal(got.observed, want["agree_obs"]) and np.array_equal(got.comparable, want["comparable_obs"])
        h.add(y)
        assert _bytes(h.result()) == ref
        with pytest.raises(EngineError, match=r"tile_pairs=65537 out of range \[0, 65536\]"):
            h.set_launch_tiles(65537)
        with pytest.raises(EngineError, match="tile_pairs=-1 out of range"):
            h.set_launch_tiles(-1)
    finally:
        h.close()


@pytest.mark.parametrize("kind", ["one_state", "elements"])
def test_the_accumulator_is_exact_at_its_limits(handle, kind):
    """N = 33 (two tiles), F = 4096: every count at 4096, the largest there is, and E = 131072, the longest contraction axis."""
    x, ns, y, want = cases.limit(kind)
    handle.set_launch_tiles(0)
    handle.set_data(x, ns)
    assert handle.last_shape()[0] == (8192 if kind == "one_state" else 131072)
    handle.add(y, agree_rep=True)
    res = handle.result()
    _equals(res, want)
    if kind == "one_state":
        off = ~np.eye(33, dtype=bool)
        assert (res.observed[off] == 4096).all() and (res.comparable[off] == 4096).all() and (res.sumsq[off] == 2 * 4096 ** 2).all()      # (two replicates)


def test_reading_takes_null_outputs(handle):
    x, ns, y, want = cases.case("n33")
    handle.set_launch_tiles(0)
    handle.set_data(x, ns)
    handle.add(y)
    lt = np.full((33, 33), -1, dtype=np.int32)
    s2 = np.full((33, 33), -1, dtype=np.int64)
    assert handle._lib.sbe_objpair_read(handle._h, None, None, None, None, lt.ctypes.data, None, s2.ctypes.data, None) == 0
    assert np.array_equal(lt, want["n_less"]) and np.array_equal(s2, want["sumsq"])
    assert handle._lib.sbe_objpair_read(handle._h, None, None, None, None, None, None, None, None) == 0


def test_set_data_refuses_and_leaves_no_data():
    x, ns, y, _want = cases.case("n65")
    h = objpair.ObjPairHandle(0)
    lib = h._lib
    try:
        def set_data(x=x, ns=ns, n=x.shape[0], f=x.shape[1]):
            x, ns = np.ascontiguousarray(x), np.ascontiguousarray(ns, dtype=np.int32)
            return lib.sbe_objpair_set_data(h._h, x.ctypes.data, n, f, ns.ctypes.data), h._last_error()

        bad_x, bad_ns = np.array(x), np.array(ns)
        bad_x[3, 2], bad_x[60, 0] = ns[2], 200
        bad_ns[5] = 33
        assert set_data(n=0)[0] == ERR_ARG and set_data(n=4097)[0] == ERR_ARG and set_data(f=0)[0] == ERR_ARG and set_data(f=4097)[0] == ERR_ARG
        code, msg = set_data(x=bad_x, ns=bad_ns)
        assert code == ERR_ARG and "n_states[5]=33 out of range [1, 32]" in msg
        code, msg = set_data(x=bad_x)
        assert code == ERR_DATA and f"x[3][2]={int(ns[2])} is neither below n_states[2]={int(ns[2])} nor 255" in msg
        # a refused call leaves the handle without data, also after a good one
        h.set_data(x, ns)
        h.add(y[:1])
        assert set_data(x=bad_x)[0] == ERR_DATA
        out = np.zeros((1,) + x.shape, dtype=np.uint8)
        assert lib.sbe_objpair_add(h._h, 1, out.ctypes.data, None) == ERR_STATE and "needs the data" in h._last_error()
        assert lib.sbe_objpair_reset(h._h) == ERR_STATE
        with pytest.raises(EngineError, match="sbe_objpair_read needs the data"):
            h.result()
        with pytest.raises(EngineError, match="no successful sbe_objpair_set_data yet"):
            h.last_shape()
        h.set_data(x, ns)                                                    # and a good one clears the accumulators
        assert h.result().n_replicates == 0 and not h.result().n_equal.any()
    finally:
        h.close()


def test_add_errors_leave_the_accumulators_alone(device):
    x, ns, y, _want = cases.case("n97")
    h = objpair.ObjPairHandle(0)
    try:
        with pytest.raises(ValueError, match="no data yet"):
            h.add(y)
        out = np.zeros((1,) + x.shape, dtype=np.uint8)
        assert h._lib.sbe_objpair_add(h._h, 1, out.ctypes.data, None) == ERR_STATE and "needs the data" in h._last_error()      # add before set_data
        h.set_data(x, ns)
        h.add(y[:2])
        before = _bytes(h.result())
        bad = np.array(y[2:4])
        bad[1, 90, 4] = ns[4]                                              # replicate 1 of the call, and a later offender behind it
        bad[1, 96, 0] = 200
        with pytest.raises(EngineError, match=rf"y_rep\[1\]\[90\]\[4\]={int(ns[4])} is neither below n_states\[4\] nor 255") as e:
            h.add(bad, agree_rep=True)
        assert e.value.code == ERR_DATA and _bytes(h.result()) == before
        bad[0, 0, 16] = 254                                                # the feature of one state
        with pytest.raises(EngineError, match=r"y_rep\[0\]\[0\]\[16\]=254 is neither"):
            h.add(bad)
        assert _bytes(h.result()) == before
        h.add(y[2:])
        assert _bytes(h.result()) == _bytes(device("n97"))
        assert h._lib.sbe_objpair_add(h._h, -1, out.ctypes.data, None) == ERR_ARG and "n=-1 is negative" in h._last_error()
        assert h._lib.sbe_objpair_add(h._h, 1, None, None) == ERR_ARG and "y_rep" in h._last_error()
        assert h._lib.sbe_objpair_add(h._h, 0, None, None) == 0
        # blocks beyond the staging limit: refused in C (split in Python); more than the counts hold: refused before that
        n = h.max_replicates() + 1
        assert n - 1 == objpair.MAX_STAGE_BYTES // objpair.replicate_bytes(97, 17, 513) == objpair.MAX_STAGE_BYTES // (97 * 17 + 128 * 384)
        assert h._lib.sbe_objpair_add(h._h, n, out.ctypes.data, None) == ERR_ARG and "exceed the 268435456 bytes one call holds" in h._last_error()
        assert h._lib.sbe_objpair_add(h._h, 2 ** 31 - 5, out.ctypes.data, None) == ERR_ARG
        assert "2147483643 replicates after 5 exceed the 2147483647" in h._last_error()
        assert _bytes(h.result()) == _bytes(device("n97"))
    finally:
        h.close()


def test_python_splits_blocks_beyond_the_staging_limit(device, monkeypatch):
    x, ns, y, _want = cases.case("n31")
    ref = device("n31")
    h = objpair.ObjPairHandle(0)
    try:
        h.set_data(x, ns)
        monkeypatch.setattr(objpair, "MAX_STAGE_BYTES", 2 * objpair.replicate_bytes(31, 17, 255, True) + 1)
        assert h.max_replicates(True) == 2
        h.add(y, agree_rep=True)
        res = h.result()
        assert _bytes(res) == _bytes(ref) and np.array_equal(res.agree_rep, ref.agree_rep)
    finally:
        h.close()


@pytest.mark.parametrize("r", [0, 1])
def test_object_pair_check_on_a_recorded_run(r):
    case = recorded_cases.case(r)
    n = case["codes"].shape[0]
    res = objpair.object_pair_check(**case, burnin=0.1, seed=SEED, device=0)
    chk = ppc.posterior_predictive_check(**case, burnin=0.1, seed=SEED, replicates=True, device=0)
    assert res.n_replicates == chk.n_samples == 54 and res.ppc.y_rep is None and res.agree_rep is None
    assert np.array_equal(res.ppc.dev_feature, chk.dev_feature) and np.array_equal(res.ppc.p_feature, chk.p_feature)
    n_states = np.full(36, case["tables"].shape[3], dtype=np.int32)
    want = orc.check(case["codes"], n_states, chk.y_rep)
    _equals(res, want)
    # the same seed's spatial check: the pairs' counts add up to its totals and to its counts per object, class by class
    rng = np.random.default_rng(40 + r)
    band, b = spatial.bands_from_costs(spatial.plane_distances(rng.random((n, 2))), n_bands=4 if r == 0 else None, knn=None if r == 0 else 6)
    sp = spatial.spatial_check(**case, band=band, n_bands=b, burnin=0.1, seed=SEED, keep=("local_agree_rep",), device=0)
    upper = np.triu(np.ones((n, n), dtype=bool), 1)
    for k in range(b):
        member = band == k
        assert int(res.observed[member & upper].sum()) == int(sp.total_obs[k]) and int(res.sum[member & upper].sum()) == int(sp.total_rep[:, k].sum())
        assert np.array_equal(np.where(member, res.observed, 0).sum(axis=1), sp.local_agree_obs[k])
        assert np.array_equal(np.where(member, res.comparable, 0).sum(axis=1), sp.local_comparable_obs[k])
        assert np.array_equal(np.where(member, res.sum, 0).sum(axis=1), sp.local_agree_rep[:, k].sum(axis=0))
    assert len(res.worst(5)) == 5 and len(res.object_table()[1]) == n
