"""patch.install(em_init=True) on the stub-imported reference: SbayesInitializer.generate_clusters_em is swapped for the
device form (sbayes_amd/em.py), here driven by a fake EM handle backed by the fp64 restatement (tests/_em_oracle.py).
Runs only where the reference exists."""
import os
import random
import sys
import warnings
from pathlib import Path

import numpy as np
import pytest

REF = "/root/reference"
pytestmark = pytest.mark.skipif(not os.path.isdir(REF), reason="reference sBayes not present")
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE / "golden"))

import _em_oracle as orc  # noqa: E402


class FakeEm:
    """EmHandle's interface on the restatement: records the z of every run."""
    created = []

    def __init__(self, x, applicable, groups_available, n_clusters, device=None):
        self.args = (x, applicable, groups_available, int(n_clusters))
        self.cost = self.scale = None
        self.geo_key = None
        self._h = True
        FakeEm.created.append(self)

    def set_geo_cost(self, cost, scale, key=None):
        self.cost, self.scale = (None, None) if cost is None else (np.asarray(cost, dtype=np.float64), float(scale))

    def run(self, z, temps):
        z = np.asarray(z, dtype=np.float64)
        if len(temps) == 0:
            return z.copy()
        self.record = {}
        self.last = orc.em_steps(*self.args, z, temps, self.cost, self.scale, record=self.record)[-1]
        return self.last

    def close(self):
        self._h = False


@pytest.fixture
def ref(monkeypatch, tmp_path):
    import make_golden as mg
    monkeypatch.setattr(mg, "WORK", tmp_path)
    from sbayes_amd import em, patch
    monkeypatch.setattr(em, "EmHandle", FakeEm)
    monkeypatch.setattr(em, "_HANDLES", {})
    FakeEm.created = []
    yield mg
    patch.uninstall()


def initializer(mg, cfg_path):
    from sbayes.experiment_setup import Experiment
    from sbayes.load_data import Data
    from sbayes.model import Model
    from sbayes.sampling.initializers import SbayesInitializer
    cwd = os.getcwd()
    os.chdir(cfg_path.parent)
    try:
        experiment = Experiment(config_file=cfg_path, experiment_name="em_patch", log=False)
        data = Data.from_config(experiment.config)
        model = Model(data, experiment.config.model)
        cfg = experiment.config.mcmc
        return SbayesInitializer(model=model, data=data, initial_size=cfg.initialization.objects_per_cluster,
                                 attempts=cfg.initialization.attempts,
                                 initial_cluster_steps=cfg.initialization._initial_cluster_steps)
    finally:
        os.chdir(cwd)


def config(mg, tag):
    if tag == "cfg1":
        return mg.write_synthetic_config("cfg1")
    from make_golden_em import geo_config
    if tag == "south_america_geo":
        return geo_config("em_patch_geo")
    return mg.stage_config(Path(REF) / "experiments" / "south_america", "em_patch_sa") / "config.yaml"


def seeded(mg, seed, fn):
    mg.seed_reference(seed)
    out = fn()
    return out, np.random.get_state(), random.getstate()


def same_rng(a, b):
    return all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


@pytest.mark.parametrize("tag", ["cfg1", "south_america", "south_america_geo"])
def test_patched_initializer_returns_the_reference_clusters_and_rng_state(ref, tag):
    from sbayes_amd import patch
    init = initializer(ref, config(ref, tag))
    plain, np_plain, py_plain = seeded(ref, 41, init.generate_clusters_em)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)            # the digest matches: no warning
        patch.install(em_init=True)
    assert patch.installed()["em_init"] is True
    assert type(init).generate_clusters_em.__module__ == "sbayes_amd.patch"
    sizes, draw = [], init.sample_n_objects_in_all_clusters
    init.sample_n_objects_in_all_clusters = lambda *a, **k: sizes.append(draw(*a, **k)) or sizes[-1]
    patched, np_patched, py_patched = seeded(ref, 41, init.generate_clusters_em)
    assert same_rng(np_patched, np_plain) and py_patched == py_plain
    fake = FakeEm.created[-1]
    assert (fake.cost is not None) == (tag == "south_america_geo")
    # the near-tie rule of test_em_oracle_cpu.py on the restatement's z from the same z0
    x, _app, avail, k = fake.args
    r = 2 * orc.z_relative_bound(x.shape[1], avail.shape[0], fake.record["ll_max"][-1], 1.0, x.shape[0],
                                 fake.record["geo_max"][-1] if fake.cost is not None else 0.0)
    zr = fake.last.astype(np.float64 if fake.cost is not None else np.float32)
    near = orc.decision_margin(zr, k, init.model.min_size, sizes[0]) <= 2 * r / (1 - r)
    differ = (patched != plain).any(axis=0)
    assert not (differ & ~near).any(), (np.flatnonzero(differ), np.flatnonzero(near))
    assert patched.shape == plain.shape and patched.dtype == bool
    patch.uninstall()
    assert type(init).generate_clusters_em.__module__ == "sbayes.sampling.initializers"
    assert patch.installed() is None


def test_handle_is_cached_per_data_object(ref):
    from sbayes_amd import patch
    init = initializer(ref, config(ref, "cfg1"))
    patch.install(em_init=True)
    for seed in (1, 2, 3):
        seeded(ref, seed, init.generate_clusters_em)
    assert len(FakeEm.created) == 1


def test_logger_path_writes_the_same_ten_samples(ref):
    from sbayes_amd import patch

    class Recorder:
        def __init__(self):
            self.samples = []

        def write_sample(self, sample):
            self.samples.append(np.array(sample.clusters.value))

    init = initializer(ref, config(ref, "south_america"))
    init.init_cluster_logger = plain_log = Recorder()
    plain, np_plain, _ = seeded(ref, 43, init.generate_clusters_em)
    patch.install(em_init=True)
    init.init_cluster_logger = patched_log = Recorder()
    patched, np_patched, _ = seeded(ref, 43, init.generate_clusters_em)
    assert len(plain_log.samples) == len(patched_log.samples) == 10
    assert same_rng(np_patched, np_plain)
    n_differ = [int((a != b).any(axis=0).sum()) for a, b in zip(plain_log.samples, patched_log.samples)]
    assert max(n_differ) <= 1, n_differ


def test_install_without_em_init_leaves_the_initializer_alone(ref):
    from sbayes_amd import patch
    import sbayes.sampling.initializers as ref_init
    original = ref_init.SbayesInitializer.__dict__["generate_clusters_em"]
    patch.install()
    assert ref_init.SbayesInitializer.__dict__["generate_clusters_em"] is original
    assert "em_init" not in patch.installed()
    patch.uninstall()
    patch.install(em_init=True)
    assert ref_init.SbayesInitializer.__dict__["generate_clusters_em"] is not original
    patch.uninstall()
    assert ref_init.SbayesInitializer.__dict__["generate_clusters_em"] is original


def test_digest_mismatch_warns(ref, monkeypatch):
    from sbayes_amd import patch
    monkeypatch.setitem(patch.MIRRORED_SOURCES, "SbayesInitializer.generate_clusters_em", "0" * 40)
    with pytest.warns(RuntimeWarning, match="SbayesInitializer.generate_clusters_em differs"):
        patch.install(em_init=True)
    patch.uninstall()


def test_whole_generate_sample_on_cfg1_has_a_finite_likelihood(ref, monkeypatch):
    from sbayes_amd import conditionals, counts, likelihood, patch, registry
    from tests._fake_engine import FakeEngine, make_engine_for_observations, make_get_engine
    engines = {}
    get_engine = make_get_engine(engines)
    for mod in (registry, likelihood, conditionals, counts):
        monkeypatch.setattr(mod, "get_engine", get_engine, raising=True)
    monkeypatch.setattr(registry, "_ENGINES", {})
    monkeypatch.setattr(registry, "engine_for_features",
                        lambda f: next((e for e in engines.values() if e.n_features == f), None)
                        or FakeEngine(np.zeros((1, f, 1), dtype=bool)))
    monkeypatch.setattr(registry, "engine_for_observations", make_engine_for_observations(engines))
    patch.install(em_init=True)
    init = initializer(ref, config(ref, "cfg1"))
    ref.seed_reference(44)
    sample = init.generate_sample(c=0)
    lh = init.model.likelihood(sample, caching=False)
    assert np.isfinite(lh)
    assert len(FakeEm.created) == 1 and sample.clusters.value.any()
