"""patch.install(gibbs_weights=True) on the stub-imported reference: GibbsSampleWeights._propose is swapped for
sbayes_amd.wgibbs.gibbs_sample_weights, here driven by the oracle-backed double of its two device calls
(tests/_wgibbs_double.py on tests/_fake_engine.py).  Runs only where the reference exists."""
import hashlib
import os
import random
import shutil
import sys
import warnings
from pathlib import Path

import numpy as np
import pytest

REF = "/root/reference"
pytestmark = pytest.mark.skipif(not os.path.isdir(REF), reason="reference sBayes not present")
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE / "golden"))


def _sha(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture
def ref(monkeypatch, tmp_path):
    import make_golden as mg
    monkeypatch.setattr(mg, "WORK", tmp_path / "work")
    (tmp_path / "work").mkdir()
    from sbayes_amd import patch
    yield mg
    patch.uninstall()


def config(mg, tag, name):
    if tag == "cfg1":
        cfg = mg.write_synthetic_config("cfg1")
        dst = mg.WORK / name
        shutil.copytree(cfg.parent, dst)
        return dst / "config.yaml"
    return mg.stage_config(Path(REF) / "experiments" / "south_america", name) / "config.yaml"


def run_chain(mg, tag, n_steps, seed, monkeypatch, patched, gibbs_source=False, decline=None):
    """n_steps of the reference's MCMCChain from its own initial sample.  Unpatched: every weights proposal goes through the
    fixture generator's recorder (the draws and the reference's p_accept; it raises where the restatement's decision on the
    same draws is another).  Patched: install(gibbs_weights=True) on the doubles."""
    import sbayes.mcmc_setup
    import sbayes.sampling.initializers as ref_init
    import sbayes.sampling.operators as ref_ops
    import sbayes.util as ref_util
    from sbayes.experiment_setup import Experiment
    from sbayes.load_data import Data
    from sbayes.model import Model
    from sbayes.sampling.initializers import SbayesInitializer
    from sbayes.sampling.mcmc_chain import MCMCChain

    import make_golden_wgibbs as gen
    from sbayes_amd import conditionals, counts, likelihood, patch, registry, wgibbs
    from tests import _wgibbs_double as double
    from tests._fake_engine import FakeEngine, make_engine_for_observations, make_get_engine

    cfg_path = config(mg, tag, f"{tag}_{'patched' if patched else 'plain'}{'_gs' if gibbs_source else ''}{'_d' if decline else ''}")
    engines, records = {}, []
    with monkeypatch.context() as mp:
        if patched:
            get_engine = make_get_engine(engines)
            for mod in (registry, likelihood, conditionals, counts):
                mp.setattr(mod, "get_engine", get_engine, raising=True)
            mp.setattr(registry, "_ENGINES", {})
            mp.setattr(registry, "engine_for_features",
                       lambda f: next((e for e in engines.values() if e.n_features == f), None)
                       or FakeEngine(np.zeros((1, f, 1), dtype=bool)))
            mp.setattr(registry, "engine_for_observations", make_engine_for_observations(engines))
            records = double.install(mp)
            if decline == "engine":
                mp.setattr(wgibbs, "engine_for", lambda op, sample: None)
            elif decline == "prior":
                mp.setattr(wgibbs, "COVERED_PRIORS", ("jeffreys",))
            patch.install(gibbs_weights=True, gibbs_source=gibbs_source)
            assert patch.installed() == {"operators": True, "gibbs_source": gibbs_source, "gibbs_weights": True}
        else:
            reference_propose = ref_ops.GibbsSampleWeights.__dict__["_propose"]

            def recording(self, sample, **kwargs):
                rec, _stats = gen.record_proposal(self, sample, np.asarray(self.model.likelihood.na_features), propose=reference_propose)
                records.append(rec)
                return sample, self.Q_GIBBS, self.Q_BACK_GIBBS
            mp.setattr(ref_ops.GibbsSampleWeights, "_propose", recording)
        try:
            np.random.seed(seed)
            random.seed(seed)
            for mod in (ref_ops, ref_init, ref_util, sbayes.mcmc_setup):
                mp.setattr(mod, "RNG", np.random.default_rng(seed), raising=True)
            cwd = os.getcwd()
            os.chdir(cfg_path.parent)
            try:
                experiment = Experiment(config_file=cfg_path, experiment_name="wgibbs_patch", log=False)
                data = Data.from_config(experiment.config)
                model = Model(data, experiment.config.model)
                cfg = experiment.config.mcmc
                init = SbayesInitializer(model=model, data=data, initial_size=cfg.initialization.objects_per_cluster,
                                         attempts=cfg.initialization.attempts,
                                         initial_cluster_steps=cfg.initialization._initial_cluster_steps)
                sample = init.generate_sample(c=0)
                chain = MCMCChain(model=model, data=data, operators=cfg.operators, sample_loggers=[])
                chain._ll = chain.likelihood(sample)
                chain._prior = chain.prior(sample)
                trace = []
                for i in range(1, n_steps + 1):
                    sample = chain.step(sample)
                    sample.i_step = i
                    trace.append((chain.previous_operator.operator_name, float(chain._ll), float(chain._prior),
                                  _sha(sample.clusters.value), _sha(sample.source.value), _sha(sample.weights.value),
                                  int(sample.weights.version), float(chain.callable_operators["gibbs_sample_weights"].last_accept_rate)))
                state = (np.random.get_state(), random.getstate(), ref_ops.RNG.bit_generator.state)
                return trace, records, engines, state
            finally:
                os.chdir(cwd)
        finally:
            if patched:
                patch.uninstall()


def same_rng(a, b):
    np_a, py_a, gen_a = a
    np_b, py_b, gen_b = b
    return all(np.array_equal(x, y) for x, y in zip(np_a, np_b)) and py_a == py_b and gen_a == gen_b


@pytest.mark.parametrize("tag,n_steps,seed,gibbs_source", [("cfg1", 150, 11, False), ("south_america", 120, 11, False),
                                                           ("south_america", 120, 12, True)])
def test_patched_sampler_follows_the_reference_chain(ref, monkeypatch, tag, n_steps, seed, gibbs_source):
    """Same operators, same clusters, source and weights at every step, the same version counter of the weights, the same
    accept rates, the three random streams in the same state at the end.  The seed is one for which no weights decision
    falls between the reference's p and the restatement's: asserted, proposal by proposal."""
    plain, ref_records, _, rng_plain = run_chain(ref, tag, n_steps, seed, monkeypatch, patched=False)
    patched, dev_records, engines, rng_patched = run_chain(ref, tag, n_steps, seed, monkeypatch, patched=True, gibbs_source=gibbs_source)
    n_weights = sum(t[0] == "GibbsSampleWeights" for t in plain)
    assert n_weights >= 10 and len(ref_records) == len(dev_records) == n_weights
    for k, (r, d) in enumerate(zip(ref_records, dev_records)):
        assert tuple(r["i12"]) == d["i12"] and np.array_equal(r["a2"], d["a2"]) and np.array_equal(r["u"], d["u"]), k
        assert np.array_equal(r["beta_ab"], d["beta_ab"]) and np.array_equal(r["w"], d["w"]), k
        assert d["w_new"].tobytes() == r["w_new"].tobytes(), k
        with np.errstate(over="ignore", invalid="ignore"):
            between = (r["u"] < r["p_accept"]) != (r["u"].astype(np.float64) < np.exp(d["terms"]["log_p"]))
        assert not between.any(), (k, np.flatnonzero(between))
        assert np.array_equal(d["accept"], r["accept"]), k
    assert [t[0] for t in patched] == [t[0] for t in plain]                     # same operators chosen
    np.testing.assert_allclose([t[1:3] for t in patched], [t[1:3] for t in plain], rtol=1e-12)
    for i, (a, b) in enumerate(zip(patched, plain)):
        assert a[3:] == b[3:], (i, a[0])                                        # clusters, source, weights, version, accept rate
    versions = [0] + [t[6] for t in plain]
    steps = [i for i, t in enumerate(plain) if t[0] == "GibbsSampleWeights"]
    assert all(versions[i + 1] - versions[i] == 2 for i in steps)               # set_value twice per proposal
    assert same_rng(rng_plain, rng_patched)
    eng = next(iter(engines.values()))
    kinds = [c[0] for c in eng.calls]
    assert kinds.count("wgibbs_pair_counts") == kinds.count("wgibbs_step") == n_weights
    assert "source_lh_by_feature" not in kinds                                  # the parent's path of this operator is not taken


@pytest.mark.parametrize("decline", ["engine", "prior"])
def test_the_reference_body_runs_where_the_device_form_declines(ref, monkeypatch, decline):
    plain, _, _, rng_plain = run_chain(ref, "cfg1", 80, 13, monkeypatch, patched=False)
    patched, dev_records, engines, rng_patched = run_chain(ref, "cfg1", 80, 13, monkeypatch, patched=True, decline=decline)
    assert any(t[0] == "GibbsSampleWeights" for t in plain) and not dev_records
    assert [t[0] for t in patched] == [t[0] for t in plain]
    assert [t[3:] for t in patched] == [t[3:] for t in plain]
    assert same_rng(rng_plain, rng_patched)
    kinds = {c[0] for e in engines.values() for c in e.calls}
    assert not {"wgibbs_pair_counts", "wgibbs_step"} & kinds


def test_install_and_uninstall(ref):
    from sbayes_amd import patch
    import sbayes.sampling.operators as ref_ops
    original = ref_ops.GibbsSampleWeights.__dict__["_propose"]
    patch.install(operators=True, gibbs_source=True)
    assert ref_ops.GibbsSampleWeights.__dict__["_propose"] is original
    assert patch.installed() == {"operators": True, "gibbs_source": True}       # no key unless the hook is on
    patch.uninstall()
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)                         # the digests match: no warning
        patch.install(gibbs_weights=True)
    assert patch.installed() == {"operators": True, "gibbs_source": False, "gibbs_weights": True}
    swapped = ref_ops.GibbsSampleWeights.__dict__["_propose"]
    assert swapped is not original and swapped.__module__ == "sbayes_amd.patch"
    assert ref_ops.GibbsSampleWeights.source_lh_by_feature.__module__ == "sbayes_amd.patch"    # operators=True is implied
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                        # (a second install compares the swapped forms' digests)
        patch.install(gibbs_weights=True)                                       # a second install swaps nothing twice
    assert ref_ops.GibbsSampleWeights.__dict__["_propose"] is swapped and patch.installed()["gibbs_weights"] is True
    patch.uninstall()
    assert ref_ops.GibbsSampleWeights.__dict__["_propose"] is original and patch.installed() is None


@pytest.mark.parametrize("name", ["GibbsSampleWeights._propose", "GibbsSampleWeights.resample_weight_for_two_components"])
def test_digest_mismatch_warns(ref, monkeypatch, name):
    from sbayes_amd import patch
    monkeypatch.setitem(patch.MIRRORED_SOURCES, name, "0" * 40)
    with pytest.warns(RuntimeWarning, match=f"{name} differs"):
        patch.install(gibbs_weights=True)
    patch.uninstall()
