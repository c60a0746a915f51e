#!/usr/bin/env python3
"""Record the reference's own cost-based geo prior (sbayes/model/prior.py: GeoPrior.__call__ and
GeoPrior.get_costs_per_object) into tests/golden/geo_prior.npz.

Runs only in the build container (needs the reference, through make_golden.py's stubs; that file is not edited).  A
GeoPrior is constructed per combination of skeleton (mst, complete_graph) x aggregation (mean, sum, max) x probability
function (exponential, sigmoid) from a GeoPriorConfig, the case's cost matrix and a stand-in network; it is called on a
stand-in sample that holds the reference's own Clusters parameter and CacheNode.

Per case `<c>`: `<c>/cost` float64 [N, N], or `<c>/xy` float64 [N, 2] whose Euclidean distances (tests/_geo_oracle.py:
euclidean_cost) are the cost; `<c>/masks` bool [B, N]; `<c>/scale`, `<c>/x0` float64 [3], the rate and the sigmoid's
inflection point per aggregation (chosen so that the sigmoid's argument stays within [-60, 10]: the reference's
log(expit(t)) is -inf below -745); `<c>/prior` float64 [2, 3, 2, B], the per-cluster values the reference left in its
cache node after GeoPrior.__call__(sample, caching=False); `<c>/per_object` float64 [3, 2, B, N], what
get_costs_per_object returned (it takes the MST whatever the skeleton); `<c>/edges_size` int64, `<c>/edges_sum`,
`<c>/edges_max` float64 [2, B]: the size, np.sum and np.max of what compute_distances_along_skeleton returned (an MST
without a non-zero edge comes back as one zero: size 1).  Deterministic: every case has its own seed.

    python tests/golden/make_golden_geo.py            # rewrites tests/golden/geo_prior.npz
"""
from __future__ import annotations

import os
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))

import make_golden as mg  # noqa: E402  (installs the reference stubs)
import _geo_oracle as orc  # noqa: E402

SKELETONS = ("mst", "complete_graph")
AGGREGATIONS = ("mean", "sum", "max")
PROBABILITY_FUNCTIONS = ("exponential", "sigmoid")


def random_masks(rng, n, sizes):
    masks = np.zeros((len(sizes), n), dtype=bool)
    for row, size in zip(masks, sizes):
        row[rng.choice(n, size=size, replace=False)] = True
    return masks


def south_america():
    """Real locations, cost from data (the reference's own network of the south_america experiment)."""
    from make_golden_em import geo_config
    from sbayes.experiment_setup import Experiment
    from sbayes.load_data import Data
    cfg_path = geo_config("south_america_geo_prior")
    cwd = os.getcwd()
    os.chdir(cfg_path.parent)
    try:
        experiment = Experiment(config_file=cfg_path, experiment_name="golden_geo", log=False)
        data = Data.from_config(experiment.config)
    finally:
        os.chdir(cwd)
    cost = np.asarray(data.geo_cost_matrix, dtype=np.float64)
    rng = np.random.default_rng(201)
    return dict(cost=cost), random_masks(rng, cost.shape[0], [8, 25, 40])


def synthetic():
    rng = np.random.default_rng(202)
    xy = rng.uniform(0, 1000, size=(1000, 2))
    return dict(xy=xy), random_masks(rng, 1000, [5, 100, 128, 129, 300])


def duplicates():
    """Integer grid coordinates: many objects share a place (zero costs) and many distances tie."""
    rng = np.random.default_rng(203)
    xy = rng.integers(0, 6, size=(120, 2)).astype(np.float64)
    return dict(xy=xy), random_masks(rng, 120, [30, 60, 120])


def ties():
    rng = np.random.default_rng(204)
    a = rng.integers(0, 4, size=(80, 80))
    cost = np.triu(a, 1)
    cost = (cost + cost.T).astype(np.float64)
    return dict(cost=cost), random_masks(rng, 80, [10, 40, 80])


def all_zero():
    rng = np.random.default_rng(205)
    return dict(cost=np.zeros((30, 30))), random_masks(rng, 30, [1, 7, 30])


def single():
    rng = np.random.default_rng(206)
    return dict(xy=rng.uniform(0, 100, size=(50, 2))), random_masks(rng, 50, [1, 1])


def pair():
    rng = np.random.default_rng(207)
    xy = rng.uniform(0, 100, size=(50, 2))
    xy[11] = xy[3]                                           # one pair in one place
    masks = random_masks(rng, 50, [2, 2])
    masks = np.concatenate([masks, np.zeros((1, 50), dtype=bool)])
    masks[2, [3, 11]] = True
    return dict(xy=xy), masks


def whole():
    rng = np.random.default_rng(208)
    return dict(xy=rng.uniform(0, 300, size=(200, 2))), np.ones((1, 200), dtype=bool)


CASES = {"south_america": south_america, "synthetic": synthetic, "duplicates": duplicates, "ties": ties, "all_zero": all_zero,
         "single": single, "pair": pair, "whole": whole}


def stand_in_sample(masks):
    from sbayes.sampling.state import CacheNode, Clusters
    clusters = Clusters(np.array(masks, dtype=bool))
    node = CacheNode(value=np.zeros(masks.shape[0]))
    node.add_input("clusters", clusters)
    return SimpleNamespace(clusters=clusters, cache=SimpleNamespace(geo_prior=node), n_objects=masks.shape[1], n_clusters=masks.shape[0])


def record(inputs, masks):
    from sbayes.config.config import GeoPriorConfig
    from sbayes.model.prior import GeoPrior
    cost = inputs["cost"] if "cost" in inputs else orc.euclidean_cost(inputs["xy"])
    lat_lon = inputs.get("xy", np.zeros((cost.shape[0], 2)))
    network = SimpleNamespace(dist_mat=cost, lat_lon=lat_lon)
    b, n = masks.shape
    # the rate and the inflection point per aggregation: the largest aggregate over masks and skeletons is 50 rates
    scale, x0 = np.ones(3), np.zeros(3)
    for a, agg in enumerate(AGGREGATIONS):
        top = max(orc.skeleton(cost, mk, sk)[agg] for mk in masks for sk in SKELETONS)
        scale[a] = top / 50 if top > 0 else 1.0
        x0[a] = 10 * scale[a]
    prior = np.empty((2, 3, 2, b))
    edges_size, edges_sum, edges_max = np.empty((2, b), dtype=np.int64), np.empty((2, b)), np.empty((2, b))
    per_object = np.empty((3, 2, b, n))
    for s, sk in enumerate(SKELETONS):
        for a, agg in enumerate(AGGREGATIONS):
            for p, pf in enumerate(PROBABILITY_FUNCTIONS):
                config = GeoPriorConfig(type="cost_based", rate=float(scale[a]), aggregation=agg, probability_function=pf,
                                        inflection_point=float(x0[a]), skeleton=sk)
                geo = GeoPrior(config=config, cost_matrix=cost, network=network)
                sample = stand_in_sample(masks)
                total = geo(sample, caching=False)
                prior[s, a, p] = sample.cache.geo_prior.value
                assert np.isclose(total, prior[s, a, p].sum())
                if s == 0:
                    for i in range(b):
                        per_object[a, p, i] = geo.get_costs_per_object(sample, i)
                if a == 0 and p == 0:
                    for i in range(b):
                        edges = np.asarray(geo.compute_distances_along_skeleton(masks[i]))
                        edges_size[s, i], edges_sum[s, i], edges_max[s, i] = edges.size, np.sum(edges), np.max(edges)
    assert np.all(np.isfinite(prior)) and np.all(np.isfinite(per_object))
    return dict(masks=masks, scale=scale, x0=x0, prior=prior, per_object=per_object, edges_size=edges_size, edges_sum=edges_sum,
                edges_max=edges_max, **inputs)


def main():
    mg.WORK.mkdir(parents=True, exist_ok=True)
    arrays = {}
    for name, make in CASES.items():
        inputs, masks = make()
        out = record(inputs, masks)
        arrays.update({f"{name}/{k}": v for k, v in out.items()})
        print(f"[golden-geo] {name}: N={masks.shape[1]} members={masks.sum(axis=1).tolist()} scale={out['scale'].tolist()}")
    path = Path(os.environ.get("SBAYES_AMD_GOLDEN_OUT", str(HERE))) / "geo_prior.npz"
    np.savez_compressed(path, **arrays)
    print(f"[golden-geo] wrote {path} ({path.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
