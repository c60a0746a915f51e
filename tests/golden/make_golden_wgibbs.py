#!/usr/bin/env python3
"""Record the reference's own Gibbs weights operator (GibbsSampleWeights._propose,
sbayes/sampling/operators.py:597-676) into tests/golden/wgibbs.npz.

Runs only in the build container (needs the reference, through make_golden.py's stubs and helpers; that file is not
edited).  Per case a reference chain runs under a fixed seed; every few steps the chain's own weights operator -- its
unchanged `_propose` -- is applied to a copy of the chain's sample, and the proposal is recorded:

  inputs    w (raw weights), has_components, the source component of every observation, i1, i2, a2, u, the beta
            parameters, alpha (per case), the NA mask (per case; for a synthetic workload its name instead)
  reference counts, w_new, log_lh_old / new, log_prior_old / new, log_q, log_q_back, p_accept, accept, the resulting
            weights, sample.weights.version before and after

The draws are captured where the reference makes them (its `random`, `stats` and `RNG` module names are wrapped while a
proposal is recorded; the calls go through to the real objects, so the streams advance as they do unrecorded).

Tie condition.  For every recorded feature the float64 restatement (tests/_wgibbs_oracle.py) must take the reference's
decision, and |log u - log p| must exceed the device band of tests/test_gpu_wgibbs.py (_wgibbs_oracle.device_band); the
reference's log p must lie within _wgibbs_oracle.reference_bound of the restatement's.  A case that fails any of them is
recorded again under the next seed; after MAX_SEEDS seeds the script aborts.

  python tests/golden/make_golden_wgibbs.py

Cases: cfg1 (50 x 30 synthetic), south_america at T = 1, south_america_mc3 (temperature 1.3, prior temperature 1.5),
south_america with the weights prior symmetric_dirichlet (concentration 0.4), jeffreys and BBS, and headline
(1000 x 200 synthetic: the NA mask comes from sbayes_amd.synthetic)."""
from __future__ import annotations

import os
import sys
from pathlib import Path

import numpy as np
import yaml

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))

import make_golden as mg  # noqa: E402  (installs the reference stubs)
import _wgibbs_oracle as orc  # noqa: E402

SOUTH_AMERICA = Path("/root/reference/experiments/south_america")
MAX_SEEDS = 8
#        tag: (proposals, chain steps between two of them)
PLAN = {"cfg1": (12, 5), "south_america": (10, 5), "south_america_mc3": (10, 5), "south_america_symdir": (6, 5),
        "south_america_jeffreys": (6, 5), "south_america_bbs": (6, 5), "headline": (3, 4)}


class TieError(AssertionError):
    pass


class _Through:
    """A module-level name of the reference with some attributes replaced; everything else is the real object's."""

    def __init__(self, real, **replaced):
        self.__dict__.update(_real=real, _replaced=replaced)

    def __getattr__(self, name):
        return self._replaced[name] if name in self._replaced else getattr(self._real, name)


def record_proposal(op, sample, na, propose=None):
    """Run the reference's _propose on `sample` (changed in place, as the reference does) and return what it drew and
    computed, checked against the restatement.  `propose`: the reference's function where the class attribute is not it
    (tests/test_wgibbs_patch_cpu.py records through a wrapper installed in its place)."""
    import sbayes.sampling.operators as ref_ops
    rec = {"lh": [], "prior": []}
    real_stats, real_rng, real_random = ref_ops.stats, ref_ops.RNG, ref_ops.random
    prior_w = op.model.prior.prior_weights

    class Frozen:
        def __init__(self, d):
            self.d = d

        def rvs(self):
            rec["a2"] = np.array(self.d.rvs(), dtype=np.float64)
            return rec["a2"].copy()

        def logpdf(self, x):
            return self.d.logpdf(x)

    def beta(a, b):
        rec["ab"] = np.stack([np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)], axis=1)
        return Frozen(real_stats.beta(a, b))

    def sample_two(population, k):
        rec["i12"] = real_random.sample(population, k)
        return list(rec["i12"])

    def uniforms(*a, **k):
        rec["u"] = real_rng.random(*a, **k)
        return rec["u"].copy()

    real_lh = type(op).__dict__["source_lh_by_feature"].__func__
    real_pointwise = prior_w.pointwise_prior
    real_resample = op.resample_weight_for_two_components

    def lh(*a):
        rec["lh"].append(np.array(real_lh(*a)))
        return rec["lh"][-1].copy()

    def pointwise(s):
        rec["prior"].append(np.array(real_pointwise(s)))
        return rec["prior"][-1].copy()

    def resample(*a, **k):
        w_new, log_q, log_q_back = real_resample(*a, **k)
        rec.update(w_new=np.array(w_new), log_q=np.array(log_q, dtype=np.float64), log_q_back=np.array(log_q_back, dtype=np.float64))
        return w_new, log_q, log_q_back

    w = sample.weights.value.copy()
    hc = np.array(sample.cache.has_components.value, dtype=bool)
    source = np.array(sample.source.value, dtype=bool)
    version = [int(sample.weights.version)]
    ref_ops.stats = _Through(real_stats, beta=beta)
    ref_ops.RNG = _Through(real_rng, random=uniforms)
    ref_ops.random = _Through(real_random, sample=sample_two)
    op.source_lh_by_feature, prior_w.pointwise_prior, op.resample_weight_for_two_components = lh, pointwise, resample
    try:
        out, q, q_back = (propose or type(op).__dict__["_propose"])(op, sample)
    finally:
        ref_ops.stats, ref_ops.RNG, ref_ops.random = real_stats, real_rng, real_random
        del op.source_lh_by_feature, prior_w.pointwise_prior, op.resample_weight_for_two_components
    assert out is sample and q == op.Q_GIBBS and q_back == op.Q_BACK_GIBBS
    version.append(int(sample.weights.version))
    T = float(op.prior_temperature)
    i1, i2 = rec["i12"]
    (lh_old, lh_new), (prior_old, prior_new) = rec["lh"], rec["prior"]
    # the reference's own expressions (operators.py:620-627) on what it computed
    p_accept = np.exp(((lh_new + prior_new) - (lh_old + prior_old) + rec["log_q_back"] - rec["log_q"]) / T)
    accept = rec["u"] < p_accept
    assert np.array_equal(sample.weights.value, np.where(accept[:, np.newaxis], rec["w_new"], w))
    assert np.isclose(op.last_accept_rate, np.mean(accept))
    has_both = np.logical_and(hc[:, i1], hc[:, i2])
    counts = np.sum(source[has_both, :, :], axis=0)[:, [i1, i2]].astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        log_p_ref = ((lh_new + prior_new) - (lh_old + prior_old) + rec["log_q_back"] - rec["log_q"]) / T

    # the restatement on the same inputs
    alpha = np.array(prior_w.concentration, dtype=np.float64)
    patterns, pid, src = orc.state_of(hc, source, na)
    assert np.array_equal(orc.pair_counts(patterns, pid, src, na, i1, i2), counts)
    assert np.array_equal(orc.beta_parameters(counts, prior_w.concentration_array, i1, i2, T), rec["ab"])
    w_out, acc, terms, w_new = orc.step(w, patterns, pid, src, na, i1, i2, rec["a2"], rec["u"], alpha, rec["ab"], T)
    assert w_new.tobytes() == rec["w_new"].tobytes(), "w_new is not the reference's bit for bit"
    if not np.array_equal(acc, accept):
        raise TieError(f"{int((acc != accept).sum())} decisions differ between the reference and the restatement")
    band = orc.device_band(terms, T)
    margin = orc.log_margin(rec["u"], terms["log_p"])
    if not (margin > band).all():
        raise TieError(f"a decision lies inside the device band: margin {margin.min():.3e}")
    finite = np.isfinite(log_p_ref) & np.isfinite(terms["log_p"])
    assert np.array_equal(np.isnan(log_p_ref), np.isnan(terms["log_p"]))
    excess = np.abs(log_p_ref - terms["log_p"])[finite] - orc.reference_bound(terms, hc.shape[0], T)[finite]
    assert (excess <= 0).all(), excess.max()
    stats = dict(d_log_p=float(np.abs(log_p_ref - terms["log_p"])[finite].max(initial=0.0)),
                 rel_margin=float(np.min(margin / np.maximum(band, 1e-300))), accepted=int(accept.sum()))
    return dict(w=w, has_components=np.packbits(hc), src=src.astype(np.int8), i12=np.array([i1, i2], dtype=np.int64),
                a2=rec["a2"], u=rec["u"].astype(np.float32), beta_ab=rec["ab"], counts=counts, w_new=rec["w_new"],
                log_lh_old=lh_old, log_lh_new=lh_new, log_prior_old=prior_old, log_prior_new=prior_new, log_q=rec["log_q"],
                log_q_back=rec["log_q_back"], p_accept=p_accept, accept=accept, w_out=sample.weights.value.copy(),
                version=np.array(version, dtype=np.int64)), stats


def record_case(tag, cfg_path: Path, seed: int, temperature=1.0, prior_temperature=1.0, workload=None):
    from sbayes.experiment_setup import Experiment
    from sbayes.load_data import Data
    from sbayes.model import Model
    from sbayes.sampling.counts import recalculate_feature_counts
    from sbayes.sampling.initializers import SbayesInitializer
    from sbayes.sampling.mcmc_chain import MCMCChain

    n_props, gap = PLAN[tag]
    cwd = os.getcwd()
    os.chdir(cfg_path.parent)
    try:
        mg.seed_reference(seed)
        experiment = Experiment(config_file=cfg_path, experiment_name=f"golden_wgibbs_{tag}", log=False)
        data = Data.from_config(experiment.config)
        model = Model(data, experiment.config.model)
        mcmc_cfg = experiment.config.mcmc
        init = SbayesInitializer(model=model, data=data, initial_size=mcmc_cfg.initialization.objects_per_cluster,
                                 attempts=mcmc_cfg.initialization.attempts,
                                 initial_cluster_steps=mcmc_cfg.initialization._initial_cluster_steps)
        sample = init.generate_sample(c=0)
        recalculate_feature_counts(data.features.values, sample)
        chain = MCMCChain(model=model, data=data, operators=mcmc_cfg.operators, sample_loggers=[], temperature=temperature,
                          prior_temperature=prior_temperature)
        chain._ll = chain.likelihood(sample)
        chain._prior = chain.prior(sample)
        op = chain.callable_operators["gibbs_sample_weights"]
        assert op.prior_temperature == prior_temperature
        na = np.array(data.features.na_values, dtype=bool)
        props, stats, i_step = [], [], 0
        for k in range(n_props):
            for _ in range(gap):
                i_step += 1
                sample = chain.step(sample)
                sample.i_step = i_step
            p, s = record_proposal(op, sample.copy(), na)
            props.append(p)
            stats.append(s)
        prior_w = model.prior.prior_weights
        n, f, c = sample.source.value.shape
        out = {f"{tag}/{key}": np.stack([p[key] for p in props]) for key in props[0]}
        out[f"{tag}/shape"] = np.array([n, f, c], dtype=np.int64)
        out[f"{tag}/prior_temperature"] = np.float64(prior_temperature)
        out[f"{tag}/temperature"] = np.float64(temperature)
        out[f"{tag}/prior_type"] = np.array(str(prior_w.prior_type.value))
        out[f"{tag}/alpha"] = np.array(prior_w.concentration, dtype=np.float64)
        out[f"{tag}/concentration_array"] = np.array(prior_w.concentration_array)
        out[f"{tag}/seed"] = np.int64(seed)
        if workload is None:
            out[f"{tag}/na"] = np.packbits(na)
        else:
            from sbayes_amd.synthetic import make_workload
            assert np.array_equal(make_workload(workload).na_values, na)
            out[f"{tag}/workload"] = np.array(workload)
        print(f"[golden-wgibbs] {tag}: seed {seed} N={n} F={f} C={c} T={prior_temperature} prior={prior_w.prior_type.value} "
              f"{n_props} proposals, {n_props * f} decisions ({sum(s['accepted'] for s in stats)} accepted), "
              f"max |d log p| {max(s['d_log_p'] for s in stats):.2e}, least margin / band {min(s['rel_margin'] for s in stats):.3g}")
        return out
    finally:
        os.chdir(cwd)


def weights_prior_config(dst_name: str, prior: dict) -> Path:
    cfg_path = mg.stage_config(SOUTH_AMERICA, dst_name) / "config.yaml"
    cfg = yaml.safe_load(cfg_path.read_text())
    cfg["model"]["prior"]["weights"] = prior
    cfg_path.write_text(yaml.safe_dump(cfg))
    return cfg_path


def with_seeds(tag, make_cfg, first_seed, **kw):
    for seed in range(first_seed, first_seed + MAX_SEEDS):
        try:
            return record_case(tag, make_cfg(), seed, **kw)
        except TieError as exc:
            print(f"[golden-wgibbs] {tag}: seed {seed} rejected ({exc}); trying the next")
    raise SystemExit(f"[golden-wgibbs] {tag}: no seed in {first_seed}..{first_seed + MAX_SEEDS - 1} meets the tie condition")


def main():
    mg.WORK.mkdir(parents=True, exist_ok=True)
    sa = lambda name: (lambda: mg.stage_config(SOUTH_AMERICA, name) / "config.yaml")      # noqa: E731
    arrays = {}
    arrays.update(with_seeds("cfg1", lambda: mg.write_synthetic_config("cfg1"), 510, workload="cfg1"))
    arrays.update(with_seeds("south_america", sa("south_america_wgibbs"), 520))
    arrays.update(with_seeds("south_america_mc3", sa("south_america_wgibbs_mc3"), 530, temperature=1.3, prior_temperature=1.5))
    arrays.update(with_seeds("south_america_symdir", lambda: weights_prior_config(
        "south_america_wgibbs_symdir", dict(type="symmetric_dirichlet", prior_concentration=0.4)), 540))
    arrays.update(with_seeds("south_america_jeffreys", lambda: weights_prior_config(
        "south_america_wgibbs_jeffreys", dict(type="jeffreys")), 550))
    arrays.update(with_seeds("south_america_bbs", lambda: weights_prior_config(
        "south_america_wgibbs_bbs", dict(type="BBS")), 560))
    arrays.update(with_seeds("headline", lambda: mg.write_synthetic_config("headline"), 570, workload="headline"))
    arrays["cases"] = np.array(list(PLAN))
    out = HERE / "wgibbs.npz"
    np.savez_compressed(out, **arrays)
    print(f"[golden-wgibbs] wrote {out} ({out.stat().st_size} bytes)")
    assert out.stat().st_size < (1 << 20)


if __name__ == "__main__":
    main()
