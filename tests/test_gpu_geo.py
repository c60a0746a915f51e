"""The cost-based geo prior on the device (sbayes_amd.geo, include/sbe_geo.h) against tests/_geo_oracle.py and against what
the reference returned (tests/golden/geo_prior.npz): integers, max and the cost to the cluster equal, sums and log priors
at the derived bounds; the device's log_expit against scipy.special's; bit-identical results for any batch position and
launch chunking; both paths of the skeleton kernel; limits and errors; the patched GeoPrior methods.

The device's exp / log1p: the ROCm documentation installed with the toolchain states no ulp bounds for them, so the
allowance is four times the largest error of the device's log_expit against scipy.special.log_expit over the fixed grid
of tests/_geo_oracle.log_expit_grid, as recorded in profiles/geo/log_expit_error.json by tools/geo_speed.py --log-expit-out
(one grid does not reach every argument; four is still far below any error of the formula)."""
import ctypes as ct
import json
import subprocess
import sys
from pathlib import Path
from types import ModuleType, SimpleNamespace

import numpy as np
import pytest

from sbayes_amd import geo
from sbayes_amd.engine import EngineError
from tests import _geo_cases as gc
from tests import _geo_oracle as orc

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
RECORDED = json.loads((REPO / "profiles" / "geo" / "log_expit_error.json").read_text())
DEVICE_LIBM = 4 * RECORDED["largest_relative_error"]
LIBM = DEVICE_LIBM + orc.HOST_LIBM                      # one side is the device, the other NumPy or the recorded reference


@pytest.fixture(scope="module")
def cases():
    return gc.load()


@pytest.fixture
def handle():
    h = geo.handle_for(0)
    h.set_launch_masks(0)
    yield h
    h.set_launch_masks(0)


def _all_priors(h, c):
    b, n = c["masks"].shape
    prior, per_object, ctc = np.empty((2, 3, 2, b)), np.empty((3, 2, b, n)), np.empty((b, n))
    for s, skeleton in enumerate(gc.SKELETONS):
        for a, agg in enumerate(gc.AGGREGATIONS):
            for p, pf in enumerate(gc.PROBABILITY_FUNCTIONS):
                prior[s, a, p] = h.prior(c["masks"], c["scale"][a], agg, pf, c["x0"][a], skeleton)
                if s == 0:
                    for i, mk in enumerate(c["masks"]):
                        per_object[a, p, i], ctc[i] = h.costs_per_object(mk, c["scale"][a], agg, pf, c["x0"][a], with_cost_to_cluster=True)
                        assert np.array_equal(ctc[i], c["cost"][mk].min(axis=0)), (agg, pf, i)
    return prior, per_object


@pytest.mark.parametrize("name", gc.CASES)
def test_device_against_oracle_and_fixture(cases, handle, name):
    c = cases[name]
    handle.set_cost(c["cost"])
    want = gc.oracle_skeletons(c)
    got = {sk: handle.skeleton_costs(c["masks"], sk) for sk in gc.SKELETONS}
    for sk in gc.SKELETONS:
        for field in ("m", "n_edges", "max"):
            assert np.array_equal(getattr(got[sk], field), want[sk][field]), (sk, field)
        assert np.array_equal(got[sk].mean, got[sk].sum / np.maximum(got[sk].n_edges, 1))
    assert np.array_equal(got["mst"].sum, want["mst"]["sum"])            # the same edges in the same order: the same bits
    err = np.abs(got["complete_graph"].sum - want["complete_graph"]["sum"])
    assert np.all(err <= orc.sum_bound(want["complete_graph"]["n_edges"]) * want["complete_graph"]["sum"])
    gc.check_skeleton_against_fixture(got, c, name)
    prior, per_object = _all_priors(handle, c)
    b = c["masks"].shape[0]
    o_prior, o_per_object = np.empty_like(prior), np.empty_like(per_object)
    for s, skeleton in enumerate(gc.SKELETONS):
        for a, agg in enumerate(gc.AGGREGATIONS):
            for p, pf in enumerate(gc.PROBABILITY_FUNCTIONS):
                o_prior[s, a, p] = orc.geo_prior(c["cost"], c["masks"], c["scale"][a], agg, pf, c["x0"][a], skeleton)
                if s == 0:
                    for i in range(b):
                        o_per_object[a, p, i] = orc.costs_per_object(c["cost"], c["masks"][i], c["scale"][a], agg, pf, c["x0"][a])[0]
    gc.check_prior(prior, o_prior, c, want, libm=LIBM, reference_form=False, label=name + " device against the oracle")
    gc.check_per_object(per_object, o_per_object, c, want["mst"], libm=LIBM, reference_form=False, label=name + " device against the oracle")
    gc.check_prior(prior, c["prior"], c, want, libm=LIBM, reference_form=True, label=name + " device against the reference")
    gc.check_per_object(per_object, c["per_object"], c, want["mst"], libm=LIBM, reference_form=True, label=name + " device against the reference")


def test_log_expit_on_the_device_against_scipy(handle):
    special = pytest.importorskip("scipy.special")
    t = orc.log_expit_grid()
    got, want = handle.log_expit(t), special.log_expit(t)
    assert np.all(np.isfinite(got)) and np.all(got <= 0)
    rel = np.abs(got - want) / np.abs(want)
    print(f"log_expit on the device against scipy.special.log_expit over {t.size} arguments: largest relative error "
          f"{float(rel.max()):.3g} at t = {float(t[np.argmax(rel)])!r} (recorded {RECORDED['largest_relative_error']:.3g}, "
          f"allowance {DEVICE_LIBM:.3g})")
    assert RECORDED["grid_points"] == t.size and RECORDED["largest_relative_error"] > 0
    assert np.all(rel <= DEVICE_LIBM)
    far = t < -746                                            # where the reference's log(expit(t)) is -inf
    assert far.any() and np.array_equal(got[far], t[far])


def test_sigmoid_far_beyond_the_inflection_point_is_finite(cases, handle):
    """The divergence from the reference under SciPy 1.15: an aggregate whose sigmoid argument lies below -745."""
    special = pytest.importorskip("scipy.special")
    c = cases["whole"]
    handle.set_cost(c["cost"])
    total = handle.skeleton_costs(c["masks"]).sum[0]
    scale, x0 = total / 5000, total / 2
    got = handle.prior(c["masks"], scale, "sum", "sigmoid", x0)[0]
    t = -(total - x0) / scale
    want = special.log_expit(t) - special.log_expit(x0 / scale)
    assert t < -2000 and np.isfinite(got)
    assert abs(got - want) <= orc.probability_bound(total, 0.0, "sigmoid", scale, x0, libm=LIBM)


def test_results_do_not_depend_on_the_batch_position_the_chunking_or_the_run(cases, handle):
    c = cases["synthetic"]
    handle.set_cost(c["cost"])
    rng = np.random.default_rng(5)
    order = np.concatenate([rng.permutation(5) for _ in range(9)])           # 45 masks: every mask at nine positions
    masks = c["masks"][order]
    kw = dict(scale=c["scale"][0], aggregation="mean", probability_function="sigmoid", inflection_point=c["x0"][0])
    first = handle.prior(masks, **kw)
    assert handle.last_shape() == (1, int(np.sum(masks.sum(axis=1) <= geo.LDS_MEMBERS))) and handle.last_kernel_ms() > 0
    alone = handle.prior(c["masks"], **kw)
    assert first.tobytes() == alone[order].tobytes()
    sk = handle.skeleton_costs(masks)
    for per_launch in (1, 7, 0):
        handle.set_launch_masks(per_launch)
        again = handle.prior(masks, **kw)
        assert handle.last_shape()[0] == (1 if per_launch == 0 else -(-45 // per_launch))
        assert again.tobytes() == first.tobytes(), per_launch
        sk2 = handle.skeleton_costs(masks)
        assert all(getattr(sk, f).tobytes() == getattr(sk2, f).tobytes() for f in ("m", "n_edges", "sum", "max", "mean"))
        for skeleton in gc.SKELETONS:
            one = handle.prior(masks, c["scale"][1], "sum", "exponential", skeleton=skeleton)
            assert one.tobytes() == handle.prior(c["masks"], c["scale"][1], "sum", "exponential", skeleton=skeleton)[order].tobytes()
    a = handle.costs_per_object(c["masks"][4], **kw)
    assert a.tobytes() == handle.costs_per_object(c["masks"][4], **kw).tobytes()


def test_a_batch_of_samples_equals_the_calls_per_mask(cases, handle):
    c = cases["south_america"]
    handle.set_cost(c["cost"])
    rng = np.random.default_rng(6)
    masks = np.zeros((4, 3, 100), dtype=bool)
    for s in range(4):
        for k in range(3):
            masks[s, k, rng.choice(100, size=rng.integers(1, 60), replace=False)] = True
    kw = dict(scale=c["scale"][1], aggregation="sum", probability_function="sigmoid", inflection_point=c["x0"][1])
    got = geo.geo_prior(masks, **kw)
    assert got.shape == (4, 3) and got.dtype == np.float64
    for s in range(4):
        for k in range(3):
            assert got[s, k] == geo.geo_prior(masks[s, k][None], **kw)[0]
    assert np.array_equal(geo.geo_prior(masks.reshape(12, 100), **kw), got.reshape(12))
    sk = handle.skeleton_costs(masks)
    assert sk.m.shape == (4, 3) and np.array_equal(sk.m, masks.sum(axis=2))
    one = geo.costs_per_object(masks[1, 2], **kw)
    assert one.shape == (100,) and np.array_equal(one, handle.costs_per_object(masks[1, 2], **kw))


def test_both_paths_of_the_skeleton_kernel_and_a_mask_of_all_objects(cases, handle):
    """m = 128 is staged in LDS, m = 129 reads its rows from memory; m = N = 1000; an asymmetric matrix on both paths."""
    c = cases["synthetic"]
    handle.set_cost(c["cost"])
    n = c["cost"].shape[0]
    rng = np.random.default_rng(7)
    masks = np.zeros((4, n), dtype=bool)
    masks[0, rng.choice(n, size=128, replace=False)] = True
    masks[1] = masks[0]
    masks[1, np.flatnonzero(~masks[0])[0]] = True
    masks[2] = True
    masks[3, rng.choice(n, size=640, replace=False)] = True
    got = handle.skeleton_costs(masks)
    assert handle.last_shape() == (1, 1) and got.m.tolist() == [128, 129, 1000, 640]
    for i, mk in enumerate(masks):
        want = orc.skeleton(c["cost"], mk, "mst")
        assert (got.m[i], got.n_edges[i], got.sum[i], got.max[i]) == (want["m"], want["n_edges"], want["sum"], want["max"]), i
    per_object, ctc = handle.costs_per_object(masks[2], c["scale"][0], "mean", "exponential", with_cost_to_cluster=True)
    assert np.all(ctc == 0) and per_object.shape == (n,)
    asym = rng.uniform(0.5, 10, size=(300, 300))
    np.fill_diagonal(asym, 0)
    handle.set_cost(asym)
    amasks = np.zeros((2, 300), dtype=bool)
    amasks[0, rng.choice(300, size=90, replace=False)] = True
    amasks[1, rng.choice(300, size=200, replace=False)] = True
    got = handle.skeleton_costs(amasks)
    for i, mk in enumerate(amasks):
        want = orc.skeleton(asym, mk, "mst")
        assert (got.n_edges[i], got.sum[i], got.max[i]) == (want["n_edges"], want["sum"], want["max"]), i
        edges = orc.scipy_mst_edges(asym[mk][:, mk])
        assert got.max[i] == edges.max() and abs(got.sum[i] - edges.sum()) <= orc.sum_bound(edges.size) * edges.sum()
    _out, ctc = handle.costs_per_object(amasks[0], 3.0, "sum", "exponential", with_cost_to_cluster=True)
    assert np.array_equal(ctc, asym[amasks[0]].min(axis=0))                   # (rows as they are: no symmetrisation here)


def test_limits_and_errors_at_the_c_boundary():
    lib = geo.load()
    h = ct.c_void_p()
    assert lib.sbe_geo_create(ct.byref(h), 0) == 0 and h
    try:
        err = lambda: lib.sbe_geo_last_error(h).decode()       # noqa: E731
        cost = np.array([[0.0, 1.0, 2.0], [1.0, 0.0, 4.0], [2.0, 4.0, 0.0]])
        masks = np.array([[1, 1, 0], [1, 1, 1]], dtype=np.uint8)
        out = np.zeros(3)
        m, ne = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int64)
        total, largest = np.zeros(2), np.zeros(2)
        sk_out = [a.ctypes.data for a in (m, ne, total, largest)]
        assert lib.sbe_geo_prior(h, masks.ctypes.data, 2, 0, 0, 0, 1.0, 0.0, out.ctypes.data) == 3            # SBE_ERR_STATE
        assert "sbe_geo_set_cost" in err()
        assert lib.sbe_geo_costs_per_object(h, masks.ctypes.data, 0, 0, 1.0, 0.0, None, out.ctypes.data) == 3
        launches, lds = ct.c_int64(), ct.c_int64()
        assert lib.sbe_geo_last_shape(h, ct.byref(launches), ct.byref(lds)) == 3
        assert lib.sbe_geo_set_cost(h, cost.ctypes.data, 32769) == 1 and "n_objects=32769" in err() and "32768" in err()
        assert lib.sbe_geo_set_cost(h, cost.ctypes.data, 0) == 1
        assert lib.sbe_geo_set_cost(h, None, 3) == 1 and "null pointer argument: cost" in err()
        bad = cost.copy()
        bad[1, 2] = np.inf
        assert lib.sbe_geo_set_cost(h, bad.ctypes.data, 3) == 4 and "cost[1][2]" in err() and "not finite" in err()         # SBE_ERR_DATA
        assert lib.sbe_geo_prior(h, masks.ctypes.data, 2, 0, 0, 0, 1.0, 0.0, out.ctypes.data) == 3            # (it holds no matrix)
        bad[1, 2] = np.nan
        assert lib.sbe_geo_set_cost(h, bad.ctypes.data, 3) == 4 and "not finite" in err()
        assert lib.sbe_geo_set_cost(h, cost.ctypes.data, 3) == 0
        assert lib.sbe_geo_skeleton(h, masks.ctypes.data, 2, 0, *sk_out) == 0
        assert (m.tolist(), ne.tolist(), total.tolist(), largest.tolist()) == ([2, 3], [1, 2], [1.0, 3.0], [1.0, 2.0])
        assert lib.sbe_geo_skeleton(h, masks.ctypes.data, 2, 1, *sk_out) == 0
        assert (ne.tolist(), total.tolist(), largest.tolist()) == ([4, 9], [2.0, 14.0], [1.0, 4.0])
        empty = masks.copy()
        empty[1] = 0
        assert lib.sbe_geo_skeleton(h, empty.ctypes.data, 2, 0, *sk_out) == 4 and "mask 1 has no member" in err()
        assert lib.sbe_geo_costs_per_object(h, empty[1].ctypes.data, 0, 0, 1.0, 0.0, None, out.ctypes.data) == 4
        assert lib.sbe_geo_skeleton(h, masks.ctypes.data, (1 << 20) + 1, 0, *sk_out) == 1 and "2^20" in err()
        assert lib.sbe_geo_skeleton(h, masks.ctypes.data, 2, 2, *sk_out) == 1 and "skeleton=2" in err()
        assert lib.sbe_geo_skeleton(h, None, 2, 0, *sk_out) == 1 and "masks" in err()
        assert lib.sbe_geo_skeleton(h, masks.ctypes.data, 2, 0, sk_out[0], None, *sk_out[2:]) == 1 and "output" in err()
        assert lib.sbe_geo_prior(h, masks.ctypes.data, 2, 0, 3, 0, 1.0, 0.0, out.ctypes.data) == 1 and "aggregation=3" in err()
        assert lib.sbe_geo_prior(h, masks.ctypes.data, 2, 0, 0, 2, 1.0, 0.0, out.ctypes.data) == 1 and "probability_function=2" in err()
        assert lib.sbe_geo_prior(h, masks.ctypes.data, 2, 0, 0, 0, 0.0, 0.0, out.ctypes.data) == 1 and "scale" in err()
        assert lib.sbe_geo_prior(h, masks.ctypes.data, 2, 0, 0, 1, 1.0, np.inf, out.ctypes.data) == 1 and "inflection_point" in err()
        assert lib.sbe_geo_prior(h, masks.ctypes.data, 2, 0, 0, 0, 1.0, 0.0, None) == 1 and "out" in err()
        assert lib.sbe_geo_set_launch_masks(h, -1) == 1 and lib.sbe_geo_set_launch_masks(h, (1 << 16) + 1) == 1
        assert lib.sbe_geo_prior(h, masks.ctypes.data, 2, 0, 1, 0, 2.0, 0.0, out.ctypes.data) == 0 and out[:2].tolist() == [-0.5, -1.5]
        assert lib.sbe_geo_last_shape(h, ct.byref(launches), ct.byref(lds)) == 0 and (launches.value, lds.value) == (1, 2)
        assert lib.sbe_geo_costs_per_object(h, masks[0].ctypes.data, 2, 0, 2.0, 0.0, None, out.ctypes.data) == 0
        assert out.tolist() == [0.0, 0.0, -0.5]                     # max(ctc, before) = 1, 1, 2 against before = 1
    finally:
        assert lib.sbe_geo_destroy(h) == 0


def test_python_layer_reports_the_state_and_data_errors():
    h = geo.GeoHandle(0)
    try:
        with pytest.raises(EngineError, match="sbe_geo_set_cost") as exc:
            h.prior(np.ones((1, 4), dtype=bool), 1.0)
        assert exc.value.code == 3
        with pytest.raises(EngineError, match="not finite") as exc:
            h.set_cost(np.array([[0.0, np.nan], [1.0, 0.0]]))
        assert exc.value.code == 4
        with pytest.raises(EngineError, match="sbe_geo_set_cost"):
            h.costs_per_object(np.ones(2, dtype=bool), 1.0)
        cost = np.array([[0.0, 2.0], [2.0, 0.0]])
        h.set_cost(cost, key="a")
        h.set_cost(np.zeros((2, 2)), key="a")                    # the same key: no upload
        assert h.prior(np.ones((1, 2), dtype=bool), 1.0)[0] == -2.0
    finally:
        h.close()


_FORK_PROBE = r"""
import json, os, sys
sys.path.insert(0, {repo!r})
import numpy as np
from sbayes_amd import _proc, geo

cost = np.abs(np.subtract.outer(np.arange(40.0), np.arange(40.0)))
masks = np.zeros((2, 40), dtype=bool)
masks[0, ::3] = True
masks[1, 5:30] = True
h = geo.handle_for(0)
h.set_cost(cost)
before = geo.geo_prior(masks, scale=3.0)
handle = h._h.value
r, w = os.pipe()
pid = os.fork()
if pid == 0:                                  # child: NO HIP call is made here
    os.close(r)
    out = dict(cache_empty=not geo._HANDLES, handle_nulled=not bool(h._h))
    for tag, fn in (("inherited", lambda: h.prior(masks, 3.0)),
                    ("create", lambda: geo.geo_prior(masks, scale=3.0)),
                    ("per_object", lambda: h.costs_per_object(masks[0], 3.0))):
        try:
            fn()
            out[tag] = "no error"
        except (_proc.ForkedWithHipError, RuntimeError) as exc:
            out[tag] = type(exc).__name__ + ": " + str(exc)
    os.write(w, json.dumps(out).encode())
    os._exit(0)
os.close(w)
child = json.loads(os.read(r, 1 << 16).decode())
_, status = os.waitpid(pid, 0)
after = geo.geo_prior(masks, scale=3.0)
print(json.dumps(dict(child=child, status=status, same=before.tobytes() == after.tobytes(), same_handle=h._h.value == handle)))
geo.release_all()
"""


def test_forked_child_forgets_the_handle():
    res = subprocess.run([sys.executable, "-c", _FORK_PROBE.format(repo=str(REPO))], capture_output=True, text=True,
                         timeout=600, cwd=str(REPO))
    assert res.returncode == 0, res.stderr[-3000:]
    out = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
    child = out["child"]
    assert out["status"] == 0 and out["same"] and out["same_handle"]
    assert child["cache_empty"] and child["handle_nulled"]
    assert child["inherited"].startswith("ForkedWithHipError") and "fork()" in child["inherited"]
    assert child["create"].startswith("ForkedWithHipError") and "forkserver" in child["create"]
    assert child["per_object"].startswith("ForkedWithHipError")


# ---- patch.install(geo_prior=True) on a stubbed sBayes: GeoPrior-shaped objects, the device behind them ------------------
class _Node:
    """The cache-node protocol GeoPrior.__call__ uses (is_outdated, what_changed, edit, value), version-tracked per cluster."""
    def __init__(self, clusters):
        self.clusters, self.value, self.seen = clusters, np.zeros(clusters.value.shape[0]), None

    def is_outdated(self):
        return self.seen is None or not np.array_equal(self.seen, self.clusters.versions)

    def what_changed(self, key, caching=True):
        assert key == "clusters"
        if not caching or self.seen is None:
            return np.arange(self.value.size)
        return np.flatnonzero(self.seen != self.clusters.versions)

    def edit(self):
        node = self

        class _Edit:
            def __enter__(self):
                return node.value

            def __exit__(self, *exc):
                node.seen = node.clusters.versions.copy()
        return _Edit()


def _stub_sample(masks):
    clusters = SimpleNamespace(value=np.array(masks, dtype=bool), versions=np.zeros(len(masks), dtype=np.int64))
    return SimpleNamespace(clusters=clusters, cache=SimpleNamespace(geo_prior=_Node(clusters)), n_objects=masks.shape[1])


@pytest.fixture
def stub_sbayes(monkeypatch):
    """An `sbayes` package of empty modules with a GeoPrior-shaped class whose own bodies only record that they ran."""
    class GeoPrior:
        ran = []

        def __init__(self, cost, scale, aggregation, probability_function, inflection_point, skeleton, prior_type="cost_based"):
            self.cost_matrix, self.scale, self.aggregation_policy = cost, scale, aggregation
            self.probability_function, self.inflection_point = probability_function, inflection_point
            self.config, self.prior_type = SimpleNamespace(skeleton=skeleton), prior_type

        def __call__(self, sample, caching=True):
            GeoPrior.ran.append("call")
            return -1.0

        def get_costs_per_object(self, sample, i_cluster):
            GeoPrior.ran.append("costs")
            return np.full(sample.n_objects, -1.0)

    names = ["sbayes", "sbayes.model", "sbayes.model.likelihood", "sbayes.model.model", "sbayes.model.prior", "sbayes.sampling",
             "sbayes.sampling.conditionals", "sbayes.sampling.counts"]
    mods = {name: ModuleType(name) for name in names}
    for name, mod in mods.items():
        if "." in name:
            setattr(mods[name.rsplit(".", 1)[0]], name.rsplit(".", 1)[1], mod)
        monkeypatch.setitem(sys.modules, name, mod)
    for name in list(sys.modules):
        if name.startswith("sbayes.") and name not in mods:
            monkeypatch.delitem(sys.modules, name)
    mods["sbayes.model.prior"].GeoPrior = GeoPrior
    from sbayes_amd import patch
    yield GeoPrior
    patch.uninstall()
    geo.handle_for(0).cost_key = None


def test_patch_routes_both_methods_to_the_device(cases, stub_sbayes):
    from sbayes_amd import patch
    c = cases["south_america"]
    sk = gc.oracle_skeletons(c)
    original = stub_sbayes.__dict__["__call__"]
    with pytest.warns(RuntimeWarning, match="GeoPrior.__call__ differs"):       # (the stub's bodies are not the mirrored revision)
        patch.install(geo_prior=True)
    assert patch.installed()["geo_prior"] is True and stub_sbayes.__dict__["__call__"] is not original
    b = c["masks"].shape[0]
    prior, per_object = np.empty((2, 3, 2, b)), np.empty((3, 2, b, c["masks"].shape[1]))
    for s, skeleton in enumerate(gc.SKELETONS):
        for a, agg in enumerate(gc.AGGREGATIONS):
            for p, pf in enumerate(gc.PROBABILITY_FUNCTIONS):
                g = stub_sbayes(c["cost"], c["scale"][a], agg, pf, c["x0"][a], skeleton)
                sample = _stub_sample(c["masks"])
                total = g(sample)
                prior[s, a, p] = sample.cache.geo_prior.value
                assert total == prior[s, a, p].sum() and not sample.cache.geo_prior.is_outdated()
                if s == 0:
                    for i in range(b):
                        per_object[a, p, i] = g.get_costs_per_object(sample, i)
    assert stub_sbayes.ran == []
    gc.check_prior(prior, c["prior"], c, sk, libm=LIBM, reference_form=True, label="patched __call__ against the reference")
    gc.check_per_object(per_object, c["per_object"], c, sk["mst"], libm=LIBM, reference_form=True,
                        label="patched get_costs_per_object against the reference")
    # a changed cluster alone goes to the device; an up-to-date cache answers by itself
    g = stub_sbayes(c["cost"], c["scale"][0], "mean", "exponential", None, "mst")
    sample = _stub_sample(c["masks"])
    first, h = g(sample), geo.handle_for(0)
    sample.clusters.value[1, np.flatnonzero(~sample.clusters.value[1])[0]] = True
    sample.clusters.versions[1] += 1
    second = g(sample)
    want = h.prior(sample.clusters.value, c["scale"][0])
    assert np.array_equal(sample.cache.geo_prior.value, want) and second == want.sum() and second != first
    ms = h.last_kernel_ms()
    assert g(sample) == second and h.last_kernel_ms() == ms
    # uncovered: the reference's own body
    delaunay = stub_sbayes(c["cost"], 1.0, "mean", "exponential", None, "delaunay")
    assert delaunay(_stub_sample(c["masks"])) == -1.0 and stub_sbayes.ran == ["call"]
    assert delaunay.get_costs_per_object(_stub_sample(c["masks"]), 0)[0] != -1.0      # (the per-object form takes the MST anyway)
    simulated = stub_sbayes(c["cost"], 1.0, "mean", "exponential", None, "mst", prior_type="simulated")
    assert simulated(_stub_sample(c["masks"])) == -1.0 and simulated.get_costs_per_object(_stub_sample(c["masks"]), 0)[0] == -1.0
    assert stub_sbayes.ran == ["call", "call", "costs"]
    patch.uninstall()
    assert stub_sbayes.__dict__["__call__"] is original and patch.installed() is None


def test_without_the_flag_the_methods_stay(stub_sbayes):
    from sbayes_amd import patch
    call, costs = stub_sbayes.__dict__["__call__"], stub_sbayes.__dict__["get_costs_per_object"]
    patch.install()
    assert stub_sbayes.__dict__["__call__"] is call and stub_sbayes.__dict__["get_costs_per_object"] is costs
    assert "geo_prior" not in patch.installed()
