#!/usr/bin/env python3
"""Record two short runs of the reference on south_america into tests/golden/diag_runs.npz: what its own
ParametersCSVLogger and ClustersLogger (sbayes/sampling/loggers.py) wrote, as the diagnostics read it.

Runs only in the build container (needs the reference, through make_golden.py's stubs and helpers; that file is not
edited).  Per run a reference chain runs under its own seed with the two loggers attached, writing `stats_K*_<run>.txt`
and `clusters_K*_<run>.txt` into the work directory; the files are then read with sbayes_amd.diag.read_stats /
read_clusters and recorded:

  names             the numeric columns of the stats files, in file order (the same for both runs)
  stats_<r>         float64 [S][P]: their values, as the text holds them (%.8g)
  cluster_names     a{k}_{object index}
  clusters_<r>      uint8 [S][ceil(K N / 8)]: the indicator columns, bit-packed along the columns (np.packbits)
  n_cluster_columns K * N
  seeds, n_steps, logging_interval

Tie condition.  tests/test_gpu_diag.py compares n_lags and flag of every column, so every column must decide with a
margin of at least tests/_diag_cases.MIN_MARGIN under the checker (tests/_diag_oracle.py) at the burn-in the test uses.
A pair of runs that does not is recorded again under the next seeds; after MAX_SEEDS tries the script aborts.

  python tests/golden/make_golden_diag.py"""
from __future__ import annotations

import os
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parent.parent))

import make_golden as mg  # noqa: E402  (installs the reference stubs)
from tests import _diag_cases as cases  # noqa: E402
from tests import _diag_oracle as orc  # noqa: E402
from sbayes_amd import diag  # noqa: E402

SOUTH_AMERICA = Path("/root/reference/experiments/south_america")
N_STEPS, LOGGING_INTERVAL, BURNIN = 1200, 20, 0.1                    # 60 samples per run: the file stays below 1 MiB
MAX_SEEDS = 8


def run_once(cfg_path: Path, seed: int, run: int):
    from sbayes.experiment_setup import Experiment
    from sbayes.load_data import Data
    from sbayes.model import Model
    from sbayes.sampling.counts import recalculate_feature_counts
    from sbayes.sampling.initializers import SbayesInitializer
    from sbayes.sampling.loggers import ClustersLogger, ParametersCSVLogger
    from sbayes.sampling.mcmc_chain import MCMCChain

    cwd = os.getcwd()
    os.chdir(cfg_path.parent)
    try:
        mg.seed_reference(seed)
        experiment = Experiment(config_file=cfg_path, experiment_name=f"golden_diag_{run}", log=False)
        data = Data.from_config(experiment.config)
        model = Model(data, experiment.config.model)
        mcmc_cfg = experiment.config.mcmc
        k = model.n_clusters
        stats_path = mg.WORK / f"stats_K{k}_{run}.txt"
        clusters_path = mg.WORK / f"clusters_K{k}_{run}.txt"
        loggers = [ParametersCSVLogger(str(stats_path), data, model, resume=False),
                   ClustersLogger(str(clusters_path), data, model, resume=False)]
        init = SbayesInitializer(model=model, data=data, initial_size=mcmc_cfg.initialization.objects_per_cluster,
                                 attempts=mcmc_cfg.initialization.attempts,
                                 initial_cluster_steps=mcmc_cfg.initialization._initial_cluster_steps)
        sample = init.generate_sample(c=0)
        recalculate_feature_counts(data.features.values, sample)
        sample.i_step = 0
        chain = MCMCChain(model=model, data=data, operators=mcmc_cfg.operators, sample_loggers=loggers)
        chain.run(n_steps=N_STEPS, logging_interval=LOGGING_INTERVAL, initial_sample=sample, log_memory_usage=False)
        chain.close_loggers()
        return stats_path, clusters_path
    finally:
        os.chdir(cwd)


def record(seed0: int):
    cfg = lambda name: mg.stage_config(SOUTH_AMERICA, name) / "config.yaml"      # noqa: E731
    out = {}
    runs = []
    for r in range(2):
        stats_path, clusters_path = run_once(cfg(f"south_america_diag_{r}"), seed0 + r, r)
        names, rows = diag.read_stats(stats_path)
        cnames, crows = diag.read_clusters(clusters_path)
        assert rows.shape[0] == crows.shape[0] == N_STEPS // LOGGING_INTERVAL
        if r == 0:
            out.update(names=np.array(names), cluster_names=np.array(cnames), n_cluster_columns=np.int64(crows.shape[1]))
        assert list(out["names"]) == names and list(out["cluster_names"]) == cnames
        out[f"stats_{r}"] = rows
        out[f"clusters_{r}"] = np.packbits(crows.astype(np.uint8), axis=1)
        runs.append(np.concatenate([rows, crows], axis=1))
    want = orc.diagnose(runs, burnin=BURNIN)
    flags = want["flag"]
    print(f"[golden-diag] seeds {seed0}, {seed0 + 1}: {runs[0].shape[0]} samples x {runs[0].shape[1]} columns per run, "
          f"{int((flags == 0).sum())} varying, {int((flags & 1 > 0).sum())} constant; least margin {want['margin'].min():.3e}, "
          f"ess {np.nanmin(want['ess']):.1f} .. {np.nanmax(want['ess'][flags == 0]):.1f}, largest n_lags {want['n_lags'].max()}")
    out.update(seeds=np.array([seed0, seed0 + 1], dtype=np.int64), n_steps=np.int64(N_STEPS), logging_interval=np.int64(LOGGING_INTERVAL))
    return out, float(want["margin"].min())


def main():
    mg.WORK.mkdir(parents=True, exist_ok=True)
    for seed0 in range(610, 610 + 2 * MAX_SEEDS, 2):
        arrays, margin = record(seed0)
        if margin >= cases.MIN_MARGIN:
            break
        print(f"[golden-diag] seeds {seed0}, {seed0 + 1} rejected: a column decides with a margin of {margin:.3e}")
    else:
        raise SystemExit("[golden-diag] no pair of seeds meets the tie condition")
    out = HERE / "diag_runs.npz"
    np.savez_compressed(out, **arrays)
    print(f"[golden-diag] wrote {out} ({out.stat().st_size} bytes)")
    assert out.stat().st_size < (1 << 20)


if __name__ == "__main__":
    main()
