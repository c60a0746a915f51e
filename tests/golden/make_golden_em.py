#!/usr/bin/env python3
"""Record the reference's own EM cluster initializer (SbayesInitializer.generate_clusters_em,
sbayes/sampling/initializers.py:93-169) into tests/golden/em_init.npz.

Runs only in the build container (needs the reference, through make_golden.py's stubs and helpers; that file is not
edited).  Under a fixed seed, per case: the inputs the device form needs (state index, applicable states, available
groups, K, min_size, the cost matrix and scale of the cost-based geo prior), the reference's z0 and total_size, its z
after steps 0, 5, ..., 45 and 49 (the float32 -- with the geo prior float64 -- arrays its own softmax returned), and
its final clusters.  The z's are captured by wrapping the module's `softmax` / `normalize` names around the reference's
unchanged method.

  python tests/golden/make_golden_em.py

Cases: cfg1 (50 x 30 x 5 synthetic, K = 2), south_america (real data, K = 3, universal + family), headline
(1000 x 200 x 10 synthetic, K = 5) and south_america_geo (south_america with `geo: {type: cost_based, rate: ...}`)."""
from __future__ import annotations

import os
import sys
from pathlib import Path

import numpy as np
import yaml

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import make_golden as mg  # noqa: E402  (installs the reference stubs)

SNAP_STEPS = list(range(0, 50, 5)) + [49]
SOUTH_AMERICA = Path("/root/reference/experiments/south_america")
GEO_RATE = 500.0


def record(tag, cfg_path: Path, seed: int):
    from sbayes.experiment_setup import Experiment
    from sbayes.load_data import Data
    from sbayes.model import Model
    import sbayes.sampling.initializers as ref_init

    cwd = os.getcwd()
    os.chdir(cfg_path.parent)
    try:
        experiment = Experiment(config_file=cfg_path, experiment_name=f"golden_em_{tag}", log=False)
        data = Data.from_config(experiment.config)
        model = Model(data, experiment.config.model)
        mcmc_cfg = experiment.config.mcmc
        init = ref_init.SbayesInitializer(model=model, data=data, initial_size=mcmc_cfg.initialization.objects_per_cluster,
                                          attempts=mcmc_cfg.initialization.attempts,
                                          initial_cluster_steps=mcmc_cfg.initialization._initial_cluster_steps)
        assert init.n_em_steps == 50
        zs, z0s, sizes = [], [], []
        real_softmax, real_normalize, real_size = ref_init.softmax, ref_init.normalize, init.sample_n_objects_in_all_clusters

        def softmax(x, axis=None):
            out = real_softmax(x, axis=axis)
            if axis == 0:
                zs.append(np.array(out))
            return out

        def normalize(x, axis=-1):
            out = real_normalize(x, axis=axis)
            if not z0s:
                z0s.append(np.array(out))
            return out

        def sample_size(*a, **k):
            sizes.append(real_size(*a, **k))
            return sizes[-1]

        ref_init.softmax, ref_init.normalize, init.sample_n_objects_in_all_clusters = softmax, normalize, sample_size
        try:
            mg.seed_reference(seed)
            clusters = init.generate_clusters_em()
        finally:
            ref_init.softmax, ref_init.normalize = real_softmax, real_normalize
        assert len(zs) == 50 and len(z0s) == 1 and len(sizes) == 1
        k = model.n_clusters
        avail = [np.ones((k, data.features.values.shape[0]), dtype=bool)]
        for conf in data.confounders.values():
            avail.append(np.asarray(conf.group_assignment, dtype=bool))
        geo = model.prior.geo_prior
        cost_based = geo.prior_type is geo.PriorTypes.COST_BASED
        import _em_oracle as orc
        out = {
            f"{tag}/x": orc.state_index(data.features.values, data.features.na_values),
            f"{tag}/applicable": np.asarray(data.features.states, dtype=bool),
            f"{tag}/groups_available": np.concatenate(avail, axis=0),
            f"{tag}/n_clusters": np.int64(k),
            f"{tag}/min_size": np.int64(model.min_size),
            f"{tag}/total_size": np.int64(sizes[0]),
            f"{tag}/z0": z0s[0],
            f"{tag}/z_steps": np.array(SNAP_STEPS, dtype=np.int64),
            f"{tag}/z": np.stack([zs[i] for i in SNAP_STEPS]),
            f"{tag}/clusters": np.asarray(clusters, dtype=bool),
        }
        if cost_based:
            out[f"{tag}/cost"] = np.asarray(geo.cost_matrix, dtype=np.float64)
            out[f"{tag}/scale"] = np.float64(geo.scale)
        print(f"[golden-em] {tag}: N={data.features.values.shape[0]} F={data.features.values.shape[1]} "
              f"S={data.features.values.shape[2]} G={out[f'{tag}/groups_available'].shape[0]} K={k} "
              f"total_size={sizes[0]} z dtype={zs[-1].dtype} geo={cost_based}")
        return out
    finally:
        os.chdir(cwd)


def geo_config(dst_name: str) -> Path:
    cfg_path = mg.stage_config(SOUTH_AMERICA, dst_name) / "config.yaml"
    cfg = yaml.safe_load(cfg_path.read_text())
    cfg["model"]["prior"]["geo"] = dict(type="cost_based", rate=GEO_RATE)
    cfg_path.write_text(yaml.safe_dump(cfg))
    return cfg_path


def main():
    sys.path.insert(0, str(HERE.parent))
    mg.WORK.mkdir(parents=True, exist_ok=True)
    arrays = {}
    arrays.update(record("cfg1", mg.write_synthetic_config("cfg1"), 31))
    arrays.update(record("south_america", mg.stage_config(SOUTH_AMERICA, "south_america_em") / "config.yaml", 32))
    arrays.update(record("headline", mg.write_synthetic_config("headline"), 33))
    arrays.update(record("south_america_geo", geo_config("south_america_em_geo"), 34))
    out = HERE / "em_init.npz"
    np.savez_compressed(out, **arrays)
    print(f"[golden-em] wrote {out} ({out.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
