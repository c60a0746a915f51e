"""patch.install(geo_prior=True) on the stub-imported reference: GeoPrior.__call__ and GeoPrior.get_costs_per_object are
swapped for the device forms (sbayes_amd/geo.py), here driven by a fake handle backed by the fp64 restatement
(tests/_geo_oracle.py).  Runs only where the reference exists."""
import os
import sys
import warnings
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

REF = "/root/reference"
pytestmark = pytest.mark.skipif(not os.path.isdir(REF), reason="reference sBayes not present")
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE / "golden"))

from tests import _geo_cases as gc  # noqa: E402
from tests import _geo_oracle as orc  # noqa: E402


class FakeGeo:
    """GeoHandle's interface on the restatement; counts what reaches it."""
    def __init__(self):
        self.cost, self.key, self.uploads, self.prior_calls, self.per_object_calls = None, None, 0, [], 0
        self._h = True

    def set_cost(self, cost, key=None):
        if key is not None and key == self.key:
            return
        self.cost, self.key = np.asarray(cost, dtype=np.float64), key
        self.uploads += 1

    def prior(self, masks, scale, aggregation, probability_function, inflection_point, skeleton):
        self.prior_calls.append(np.array(masks))
        names = [str(getattr(v, "value", v)) for v in (aggregation, probability_function, skeleton)]
        return orc.geo_prior(self.cost, masks, scale, names[0], names[1], inflection_point, names[2])

    def costs_per_object(self, mask, scale, aggregation, probability_function, inflection_point):
        self.per_object_calls += 1
        names = [str(getattr(v, "value", v)) for v in (aggregation, probability_function)]
        return orc.costs_per_object(self.cost, mask, scale, names[0], names[1], inflection_point)[0]


@pytest.fixture
def ref(monkeypatch):
    import make_golden  # noqa: F401  (installs the reference stubs)
    from sbayes_amd import geo, patch
    fake = FakeGeo()
    monkeypatch.setattr(geo, "handle_for", lambda device=0: fake)
    yield fake
    patch.uninstall()


def make_prior(c, agg, pf, skeleton, a):
    from sbayes.config.config import GeoPriorConfig
    from sbayes.model.prior import GeoPrior
    config = GeoPriorConfig(type="cost_based", rate=float(c["scale"][a]), aggregation=agg, probability_function=pf,
                            inflection_point=float(c["x0"][a]), skeleton=skeleton)
    return GeoPrior(config=config, cost_matrix=c["cost"], network=SimpleNamespace(dist_mat=c["cost"], lat_lon=np.zeros((len(c["cost"]), 2))))


def make_sample(masks):
    from make_golden_geo import stand_in_sample
    return stand_in_sample(masks)


@pytest.mark.parametrize("name", ["south_america", "duplicates", "pair"])
def test_patched_methods_leave_what_the_reference_would_have_written(ref, name):
    from sbayes_amd import patch
    import sbayes.model.prior as ref_prior
    c = gc.load()[name]
    sk = gc.oracle_skeletons(c)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)            # the digests match: no warning
        patch.install(geo_prior=True)
    assert patch.installed()["geo_prior"] is True
    assert ref_prior.GeoPrior.__call__.__module__ == "sbayes_amd.patch"
    b = c["masks"].shape[0]
    prior, per_object = np.empty((2, 3, 2, b)), np.empty((3, 2, b, c["masks"].shape[1]))
    for s, skeleton in enumerate(gc.SKELETONS):
        for a, agg in enumerate(gc.AGGREGATIONS):
            for p, pf in enumerate(gc.PROBABILITY_FUNCTIONS):
                geo_prior = make_prior(c, agg, pf, skeleton, a)
                sample = make_sample(c["masks"])
                total = geo_prior(sample)
                prior[s, a, p] = sample.cache.geo_prior.value
                assert total == prior[s, a, p].sum() and not sample.cache.geo_prior.is_outdated()
                if s == 0:
                    for i in range(b):
                        per_object[a, p, i] = geo_prior.get_costs_per_object(sample, i)
    assert len(ref.prior_calls) == 12 and ref.per_object_calls == 6 * b and ref.uploads == 1
    gc.check_prior(prior, c["prior"], c, sk, libm=orc.HOST_LIBM, reference_form=True, label=name)
    gc.check_per_object(per_object, c["per_object"], c, sk["mst"], libm=orc.HOST_LIBM, reference_form=True, label=name)
    patch.uninstall()
    assert ref_prior.GeoPrior.__call__.__module__ == "sbayes.model.prior" and patch.installed() is None


def test_only_the_changed_clusters_go_to_the_device(ref):
    from sbayes_amd import patch
    c = gc.load()["south_america"]
    patch.install(geo_prior=True)
    geo_prior = make_prior(c, "mean", "exponential", "mst", 0)
    sample = make_sample(c["masks"])
    first = geo_prior(sample)
    assert [m.shape[0] for m in ref.prior_calls] == [3]
    assert geo_prior(sample) == first and len(ref.prior_calls) == 1           # up to date: the cache answers
    with sample.clusters.edit_group(1) as cluster:
        cluster[np.flatnonzero(~cluster)[0]] = True
    second = geo_prior(sample)
    assert [m.shape[0] for m in ref.prior_calls] == [3, 1] and np.array_equal(ref.prior_calls[1][0], sample.clusters.value[1])
    want = orc.geo_prior(c["cost"], sample.clusters.value, c["scale"][0], "mean", "exponential")
    assert np.array_equal(sample.cache.geo_prior.value, want) and second == want.sum() and second != first


def test_uncovered_priors_run_the_reference_body(ref):
    from sbayes_amd import patch
    from sbayes.config.config import GeoPriorConfig
    from sbayes.model.prior import GeoPrior
    c = gc.load()["pair"]
    network = SimpleNamespace(dist_mat=c["cost"], lat_lon=np.zeros((50, 2)))
    patch.install(geo_prior=True)
    sample = make_sample(c["masks"])
    uniform = GeoPrior(config=GeoPriorConfig(type="uniform"), cost_matrix=c["cost"], network=network)
    assert uniform(sample) == 0.0 and np.array_equal(uniform.get_costs_per_object(sample, 0), np.zeros(50))
    delaunay = GeoPrior(config=GeoPriorConfig(type="cost_based", rate=1.0, skeleton="delaunay"), cost_matrix=c["cost"], network=network)
    with pytest.raises((NameError, AttributeError, ImportError)):          # the reference's own body: pysal is not installed
        delaunay(sample)
    assert not ref.prior_calls and ref.uploads == 0
    assert delaunay.get_costs_per_object(sample, 0).shape == (50,) and ref.per_object_calls == 1       # (the MST whatever the skeleton)


def test_without_the_flag_nothing_changes_and_a_changed_body_warns(ref, monkeypatch):
    from sbayes_amd import patch
    import sbayes.model.prior as ref_prior
    call, costs = ref_prior.GeoPrior.__dict__["__call__"], ref_prior.GeoPrior.__dict__["get_costs_per_object"]
    patch.install()
    assert ref_prior.GeoPrior.__dict__["__call__"] is call and ref_prior.GeoPrior.__dict__["get_costs_per_object"] is costs
    assert "geo_prior" not in patch.installed()
    patch.uninstall()
    monkeypatch.setitem(patch.MIRRORED_SOURCES, "GeoPrior.get_costs_per_object", "0" * 40)
    with pytest.warns(RuntimeWarning, match="GeoPrior.get_costs_per_object differs.*re-check sbayes_amd/geo.py"):
        patch.install(geo_prior=True)
    assert ref_prior.GeoPrior.__dict__["__call__"] is not call
    patch.uninstall()
    assert ref_prior.GeoPrior.__dict__["__call__"] is call and ref_prior.GeoPrior.__dict__["get_costs_per_object"] is costs
