"""The pairwise posterior predictive check on the device (sbayes_amd.pairppc, include/sbe_pairppc.h) against
tests/_pairppc_oracle.py on the cases of tests/_pairppc_cases.py: the observed statistic equal to the screening's byte for byte,
every replicated statistic at the screening's bound, the counts and sums bit for bit a host recomputation from the device's own
statistics, the counts against the oracle's up to the replicates that lie within the bound of a tie; the planted replicates;
bit-identical reads for any split of the replicates, any launch tiles, with and without stat_rep, after a reset; errors; and
pairwise_check end to end on the recorded runs.

Worst observed ratio of |device - oracle| to the bound over these cases (MI355X): see DESIGN.md section 25."""
import numpy as np
import pytest

from sbayes_amd import assoc, pairppc, ppc
from sbayes_amd.engine import EngineError
from tests import _assoc_oracle as ao
from tests import _pairppc_cases as cases
from tests import _pairppc_oracle as orc
from tests import _ppc_cases as ppc_cases

pytestmark = pytest.mark.gpu
FIELDS = ("stat_obs", "dof_obs", "n_obs", "valid_obs") + orc.INT_FIELDS + ("sum", "sumsq")
ERR_ARG, ERR_STATE, ERR_DATA = 1, 3, 4


def _bytes(res):
    return b"".join(np.ascontiguousarray(getattr(res, k)).tobytes() for k in FIELDS) + str(res.n_replicates).encode()


@pytest.fixture(scope="module")
def handle():
    h = pairppc.PairHandle(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def device(handle):
    """name -> the device's result of the case with all replicates in one add call and stat_rep kept; computed once."""
    done = {}

    def get(name):
        if name not in done:
            x, ns, y, _want = cases.case(name)
            handle.set_launch_tiles(0)
            handle.set_data(x, ns)
            handle.add(y, stat_rep=True)
            done[name] = handle.result()
        return done[name]
    return get


def _check_counts(got, want, label):
    """The rule of the oracle's docstring: a count differs from the oracle's by at most the replicates near a tie."""
    near = orc.near(want)
    for k in ("n_greater", "n_equal", "n_less"):
        off = np.abs(got[k].astype(np.int64) - want[k])
        print(f"{label}: {k} differs from the oracle's in {int((off > 0).sum()) // 2} pairs, {int(near.sum()) // 2} replicates lie near a tie")
        assert (off <= near).all(), k


@pytest.mark.parametrize("name", list(cases.CASES))
def test_a_case_against_the_screening_and_the_oracle(device, name):
    x, ns, y, want = cases.case(name)
    res = device(name)
    t_n = y.shape[0]
    assert res.n_replicates == t_n and res.stat_rep.shape == (t_n,) + want["stat_obs"].shape
    # the observed statistic is the screening's, byte for byte
    screen = assoc.feature_association(x, ns, device=0)
    for ours, theirs in (("stat_obs", "statistic"), ("dof_obs", "dof"), ("n_obs", "n"), ("valid_obs", "valid")):
        assert getattr(res, ours).tobytes() == getattr(screen, theirs).tobytes(), ours
    assert np.array_equal(res.valid_obs, want["valid_obs"]) and np.array_equal(res.dof_obs, want["dof_obs"]) and np.array_equal(res.n_obs, want["n_obs"])
    # every replicated statistic at the screening's bound, its degenerate class the oracle's
    live = want["valid_obs"][None] & np.ones((t_n, 1, 1), dtype=bool)
    assert np.array_equal(res.stat_rep, res.stat_rep.transpose(0, 2, 1)) and not res.stat_rep[~live].any()
    bound = ao.statistic_bound(want["R_rep"], want["C_rep"])
    err = np.abs(res.stat_rep - want["stat_rep"])
    ratio = err[live] / np.maximum(bound[live] * want["stat_rep"][live], ao.DBL_MIN)
    print(f"{name}: {int(live.sum()) // 2} replicated statistics, worst |device - oracle| / bound = {float(ratio.max()) if ratio.size else 0.0:.3g}")
    assert (err <= bound * want["stat_rep"]).all()
    degenerate = live & (want["dof_rep"] == 0)
    assert not res.stat_rep[degenerate].any() and np.array_equal(res.n_degenerate, want["n_degenerate"])
    # counts and sums: bit for bit the contract's loop over the device's own statistics, one replicate after the other
    again = orc.accumulate(res.stat_obs, res.valid_obs, res.stat_rep, want["dof_rep"])
    for k in orc.INT_FIELDS + ("sum", "sumsq"):
        assert getattr(res, k).tobytes() == again[k].astype(getattr(res, k).dtype).tobytes(), k
    _check_counts({k: getattr(res, k) for k in orc.INT_FIELDS}, want, name)
    p = res.p_value()
    assert ((p[res.valid_obs] >= 0) & (p[res.valid_obs] <= 1)).all() and np.isnan(p[~res.valid_obs]).all()


@pytest.mark.parametrize("name", [n for n in cases.CASES if n != "one_object"])
def test_the_planted_replicates(device, name):
    x, ns, y, want = cases.case(name)
    res = device(name)
    v = res.valid_obs
    # the data as a replicate ties with itself, bit for bit
    assert res.stat_rep[cases.SAME].tobytes() == res.stat_obs.tobytes() and (res.n_equal[v] >= 1).all()
    # a constant feature: degenerate on its pairs, s = 0
    c = cases.CONSTANT
    assert v[c].any() and not res.stat_rep[cases.DEGENERATE][c].any() and np.array_equal(res.n_degenerate[c] >= 1, v[c])
    # the labels of a binary feature swapped: the statistic of the data within the bound
    s = cases.SWAPPED
    bound = ao.statistic_bound(want["R_obs"], want["C_obs"])[s]
    assert v[s].any() and (np.abs(res.stat_rep[cases.SWAP][s] - res.stat_obs[s]) <= bound * res.stat_obs[s]).all()


@pytest.mark.parametrize("name", [n for n in cases.CASES if n != "one_object"])
def test_both_forms_walk_all_replicates_of_a_call_to_the_same_bits(device, name):
    """The sequential form keeps its accumulators in LDS across the replicates of a call, the spread form holds the statistics
    back: each is forced here on all replicates in one call, at every S_pad, with NA and ragged tiles."""
    x, ns, y, _want = cases.case(name)
    ref, ref_rep = _bytes(device(name)), device(name).stat_rep
    h = pairppc.PairHandle(0)
    try:
        h.set_data(x, ns)
        for form in ("sequential", "spread"):
            h.set_form(form)
            h.reset()
            rep = h.add(y, stat_rep=True)
            assert _bytes(h.result()) == ref and rep.tobytes() == ref_rep.tobytes(), form
            h.reset()
            h.add(y[:3])
            h.add(y[3:])
            assert _bytes(h.result()) == ref, form
        with pytest.raises(EngineError, match="form=3 is none of"):
            h._check(h._lib.sbe_pairppc_set_form(h._h, 3))
    finally:
        h.close()


@pytest.mark.parametrize("name", ["s2", "s8", "s32", "below_spread", "at_spread"])
def test_reads_do_not_depend_on_the_split_the_tiles_or_the_statistics(device, name):
    """(Left to itself the unit takes the sequential form for a call of one replicate and from 8192 tile pairs on, the spread
    form otherwise: the splits and the two wide cases cross that choice as well.)"""
    x, ns, y, _want = cases.case(name)
    ref = _bytes(device(name))
    t_n = y.shape[0]
    h = pairppc.PairHandle(0)
    try:
        h.set_data(x, ns)
        assert h.last_shape()[1] == {"below_spread": 8128, "at_spread": 8256}.get(name, h.last_shape()[1])
        for split in ((3, t_n - 3), (1,) * t_n):
            h.reset()
            at = 0
            for n in split:
                h.add(y[at:at + n])
                at += n
            assert _bytes(h.result()) == ref, split
        for tiles in (1, 2, 5) if name not in cases.WIDE else (1000, 5000):
            h.set_launch_tiles(tiles)
            h.reset()
            h.add(y, stat_rep=(tiles in (2, 5000)))
            assert h.last_shape()[2] == -(-h.last_shape()[1] // tiles)
            assert _bytes(h.result()) == ref, tiles
        h.set_launch_tiles(0)
        h.reset()
        assert not any(getattr(h.result(), k).any() for k in orc.INT_FIELDS + ("sum", "sumsq")) and h.result().n_replicates == 0
        h.add(y)
        assert _bytes(h.result()) == ref
    finally:
        h.close()


def test_errors_leave_the_accumulators_alone():
    x, ns, y, _want = cases.case("s8")
    h = pairppc.PairHandle(0)
    try:
        out = np.zeros((1,) + y.shape[1:], dtype=np.uint8)
        assert h._lib.sbe_pairppc_add(h._h, 1, out.ctypes.data, None) == ERR_STATE and "needs the data" in h._last_error()
        with pytest.raises(ValueError, match="no data yet"):
            h.add(y)
        h.set_data(x, ns)
        h.add(y[:2])
        before = _bytes(h.result())
        bad = np.array(y[2:5])
        bad[1, 200, 4] = ns[4]                                             # replicate 2 of 3 (index 1), and a later offender behind it
        bad[2, 0, 0] = 200
        with pytest.raises(EngineError, match=rf"y_rep\[1\]\[200\]\[4\]={int(ns[4])} is neither below n_states\[4\] nor 255") as e:
            h.add(bad)
        assert e.value.code == ERR_DATA and _bytes(h.result()) == before
        h.add(y[2:])
        ref = pairppc.PairHandle(0)
        try:
            ref.set_data(x, ns)
            ref.add(y)
            assert _bytes(h.result()) == _bytes(ref.result())
        finally:
            ref.close()
        # blocks beyond the staging limit: refused in C, split in Python
        each = pairppc.replicate_bytes(*x.shape)
        n = pairppc.MAX_STAGE_BYTES // each + 1
        assert h.max_replicates() == n - 1
        assert h._lib.sbe_pairppc_add(h._h, n, out.ctypes.data, None) == ERR_ARG and "exceed the 268435456 bytes one call holds" in h._last_error()
        assert h._lib.sbe_pairppc_add(h._h, -1, out.ctypes.data, None) == ERR_ARG
        assert h._lib.sbe_pairppc_add(h._h, 1, None, None) == ERR_ARG
        with pytest.raises(EngineError, match="tile_pairs=-1 out of range"):
            h.set_launch_tiles(-1)
    finally:
        h.close()


def test_python_splits_blocks_beyond_the_staging_limit(monkeypatch):
    x, ns, y, _want = cases.case("s16")
    h = pairppc.PairHandle(0)
    try:
        h.set_data(x, ns)
        h.add(y, stat_rep=True)
        ref, ref_rep = _bytes(h.result()), h.result().stat_rep
        calls = []
        real = h._lib.sbe_pairppc_add

        class Counting:
            def __getattr__(self, name):
                return getattr(h_lib, name)

            def sbe_pairppc_add(self, handle, n, *rest):
                calls.append(n)
                return real(handle, n, *rest)
        h_lib = h._lib
        monkeypatch.setattr(pairppc, "MAX_STAGE_BYTES", 3 * pairppc.replicate_bytes(*x.shape, True) + 1)
        h._lib = Counting()
        h.reset()
        rep = h.add(y, stat_rep=True)
        h._lib = h_lib
        assert calls == [3, 3, 1] and _bytes(h.result()) == ref and rep.tobytes() == ref_rep.tobytes()
    finally:
        h.close()


@pytest.mark.parametrize("r", [0, 1])
def test_pairwise_check_on_a_recorded_run(r):
    case = ppc_cases.recorded(r)
    res = pairppc.pairwise_check(**case, burnin=0.1, seed=ppc_cases.SEED, device=0)
    chk = ppc.posterior_predictive_check(**case, burnin=0.1, seed=ppc_cases.SEED, replicates=True, device=0)
    assert res.n_replicates == chk.n_samples == 54 and res.ppc.y_rep is None
    assert np.array_equal(res.ppc.dev_feature, chk.dev_feature) and np.array_equal(res.ppc.p_feature, chk.p_feature)
    n_states = np.full(36, case["tables"].shape[3], dtype=np.int32)
    want = orc.check(case["codes"], n_states, chk.y_rep)
    assert np.array_equal(res.valid_obs, want["valid_obs"]) and np.array_equal(res.dof_obs, want["dof_obs"])
    assert np.array_equal(res.n_degenerate, want["n_degenerate"])
    assert np.array_equal(res.n_greater + res.n_equal + res.n_less, 54 * want["valid_obs"])
    _check_counts({k: getattr(res, k) for k in orc.INT_FIELDS}, want, f"run {r}")
    p = res.p_value()
    v = res.valid_obs
    assert v.sum() > 200 and ((p[v] >= 0) & (p[v] <= 1)).all()
    terms = 54 * 2.0 ** -52 + ao.statistic_bound(5, 5)
    assert (np.abs(res.sum - want["sum"]) <= terms * want["sum"]).all()
