#!/usr/bin/env python3
"""Host time of one GibbsSampleWeights._propose call with every engine call answered in O(1): the reference's own body
under patch.install(operators=True, gibbs_source=True) (the parent path) against sbayes_amd.wgibbs.gibbs_sample_weights
under install(..., gibbs_weights=True).  BUILD CONTAINER ONLY (needs the reference, imported through the stubs of
tests/golden/_ref_stubs.py); writes profiles/wgibbs/wgibbs_host.json.

Method, per shape (cfg1 50 x 30, south_america 100 x 36, headline 1000 x 200: the shapes of tests/golden/host_residual.json):
the REAL reference sampler runs a seeded chain on the oracle-backed engine double (tests/_fake_engine.py, and
tests/_wgibbs_double.py for the two new calls), once per side (`same_chain` says whether both sides followed the same
Markov chain: the same operators and the same weights after every step -- they do unless a uniform fell between the two
sides' acceptance probabilities, which differ by the float32 rounding of the parent's likelihood sums).  Around every call of the weights operator's `_propose` a clock runs;
the time spent INSIDE the doubles (every public method of the engine double, the two new calls) is measured and
subtracted, so what remains is the host's own work: proposal logic, RNG, SciPy, the bind's bookkeeping, argument
marshalling.  Every proposal's time is the least of its occurrences over --runs runs of the same deterministic chain; the
figure per shape is the mean over the proposals.

Expectation (from the issue that asked for the device form): the new figure is at most half the parent's at every shape
-- half because tests/golden/host_residual.json records 27 % day-to-day drift of this container, so a smaller gain could
not be told from noise.  `met` says whether it was.
    python tools/wgibbs_host.py [--steps-small 400] [--steps-headline 120] [--runs 3] [--out profiles/wgibbs/wgibbs_host.json]"""
from __future__ import annotations

import argparse
import gc
import json
import os
import platform
import random
import sys
import time
from pathlib import Path
from unittest import mock

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests" / "golden"))

import make_golden as mg  # noqa: E402  (installs the stubs, imports the reference)

from tests import _wgibbs_double as double  # noqa: E402
from tests._fake_engine import FakeEngine, make_engine_for_observations, make_get_engine  # noqa: E402

SOUTH_AMERICA = Path("/root/reference/experiments/south_america")
INSIDE = [0.0, 0]                                         # seconds spent inside the doubles; nesting depth


def clocked(fn):
    def inner(*a, **k):
        if INSIDE[1]:                                     # a double's method calling another: the outer call's clock runs
            return fn(*a, **k)
        INSIDE[1] = 1
        t0 = time.perf_counter()
        try:
            return fn(*a, **k)
        finally:
            INSIDE[0] += time.perf_counter() - t0
            INSIDE[1] = 0
    inner.__name__ = getattr(fn, "__name__", "clocked")
    return inner


class ClockedEngine(FakeEngine):
    pass


for _n in dir(FakeEngine):
    if not _n.startswith("_") and callable(getattr(FakeEngine, _n)) and not isinstance(FakeEngine.__dict__.get(_n), property):
        setattr(ClockedEngine, _n, clocked(getattr(FakeEngine, _n)))


def run(cfg_path: Path, n_steps: int, seed: int, gibbs_weights: bool):
    import sbayes.mcmc_setup
    import sbayes.sampling.initializers as ref_init
    import sbayes.sampling.operators as ref_ops
    import sbayes.util as ref_util
    from sbayes.experiment_setup import Experiment
    from sbayes.load_data import Data
    from sbayes.model import Model
    from sbayes.sampling.initializers import SbayesInitializer
    from sbayes.sampling.mcmc_chain import MCMCChain
    from sbayes_amd import conditionals, counts, likelihood, patch, registry, wgibbs

    engines = {}
    get_engine = make_get_engine(engines, cls=ClockedEngine)
    records = []
    patches = [mock.patch.object(mod, "get_engine", get_engine) for mod in (registry, likelihood, conditionals, counts)]
    patches += [mock.patch.object(registry, "_ENGINES", {}),
                mock.patch.object(registry, "engine_for_features",
                                  lambda f: next((e for e in engines.values() if e.n_features == f), None)
                                  or ClockedEngine(np.zeros((1, f, 1), dtype=bool))),
                mock.patch.object(registry, "engine_for_observations", make_engine_for_observations(engines)),
                mock.patch.object(wgibbs, "pair_counts", clocked(double.pair_counts)),
                mock.patch.object(wgibbs, "step", clocked(double.make_step(records)))]
    patches += [mock.patch.object(mod, "RNG", np.random.default_rng(seed)) for mod in (ref_ops, ref_init, ref_util, sbayes.mcmc_setup)]
    for p in patches:
        p.start()
    patch.install(operators=True, gibbs_source=True, gibbs_weights=gibbs_weights)
    times = []
    installed = ref_ops.GibbsSampleWeights.__dict__["_propose"]

    def timed_propose(self, sample, **kwargs):
        gc.disable()
        inside0, t0 = INSIDE[0], time.perf_counter()
        try:
            return installed(self, sample, **kwargs)
        finally:
            times.append((time.perf_counter() - t0) - (INSIDE[0] - inside0))
            gc.enable()

    ref_ops.GibbsSampleWeights._propose = timed_propose
    cwd = os.getcwd()
    os.chdir(cfg_path.parent)
    try:
        np.random.seed(seed)
        random.seed(seed)
        experiment = Experiment(config_file=cfg_path, experiment_name="wgibbs_host", log=False)
        data = Data.from_config(experiment.config)
        model = Model(data, experiment.config.model)
        cfg = experiment.config.mcmc
        init = SbayesInitializer(model=model, data=data, initial_size=cfg.initialization.objects_per_cluster,
                                 attempts=cfg.initialization.attempts, initial_cluster_steps=cfg.initialization._initial_cluster_steps)
        sample = init.generate_sample(c=0)
        chain = MCMCChain(model=model, data=data, operators=cfg.operators, sample_loggers=[])
        chain._ll = chain.likelihood(sample)
        chain._prior = chain.prior(sample)
        trace = []
        for i in range(1, n_steps + 1):
            sample = chain.step(sample)
            sample.i_step = i
            trace.append((chain.previous_operator.operator_name, sample.weights.value.tobytes()))
        return times, trace
    finally:
        os.chdir(cwd)
        ref_ops.GibbsSampleWeights._propose = installed
        patch.uninstall()
        for p in reversed(patches):
            p.stop()


def measure(tag, make_cfg, n_steps, seed, runs):
    best = {False: None, True: None}
    traces = {}
    for r in range(runs):
        for side in (False, True):                          # the two sides alternate: drift of the host hits both
            times, trace = run(make_cfg(f"{tag}_{int(side)}_{r}"), n_steps, seed, side)
            traces.setdefault(side, trace)
            assert trace == traces[side]
            best[side] = times if best[side] is None else [min(a, b) for a, b in zip(best[side], times)]
    # (the same chain unless a uniform fell between the two sides' p: the parent's likelihood sums are rounded to float32,
    #  the device form's log ratio is float64 -- at N = 1000 that is up to 1e-2 of p)
    same_chain = traces[False] == traces[True]
    parent, new = (float(np.mean(best[s])) * 1e3 for s in (False, True))
    return dict(shape=tag, steps=n_steps, proposals=dict(parent=len(best[False]), new=len(best[True])), same_chain=same_chain, runs=runs,
                parent_ms_per_call=round(parent, 4),
                new_ms_per_call=round(new, 4), ratio=round(new / parent, 4), met=bool(new <= 0.5 * parent))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps-small", type=int, default=400)
    ap.add_argument("--steps-headline", type=int, default=120)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", type=Path, default=REPO / "profiles" / "wgibbs" / "wgibbs_host.json")
    args = ap.parse_args()
    mg.WORK.mkdir(parents=True, exist_ok=True)

    def synthetic(name):
        def make(dst_name):
            cfg = mg.write_synthetic_config(name)
            return cfg
        return make
    shapes = [("cfg1", synthetic("cfg1"), args.steps_small), ("south_america", lambda d: mg.stage_config(SOUTH_AMERICA, d) / "config.yaml", args.steps_small),
              ("headline", synthetic("headline"), args.steps_headline)]
    result = dict(what="host milliseconds per GibbsSampleWeights._propose call with every engine call answered in O(1): the parent "
                       "path (install(operators=True, gibbs_source=True)) and the device form's host side (+ gibbs_weights=True); "
                       "see tools/wgibbs_host.py",
                  host=dict(machine=platform.machine(), cpus=os.cpu_count(), python=platform.python_version(), numpy=np.__version__),
                  expectation="new_ms_per_call <= 0.5 * parent_ms_per_call at every shape",
                  shapes=[measure(tag, make, steps, 21, args.runs) for tag, make, steps in shapes])
    result["met_everywhere"] = all(s["met"] for s in result["shapes"])
    print(json.dumps(result))
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
